"""ScalarTransportStepper on the device against the NumPy restatement (tests/_scalar_ref.py), bit for bit: the passive scalar next to
the plain stepper, walled cases with every scalar rule, buoyancy, the native run loop, and the refusals."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import (EquilibriumBC, ExtrapolationOutflowBC, FullwayBounceBackBC, HalfwayBounceBackBC, HybridBC,
                                                 RegularizedBC, ScalarAdiabaticBC, ScalarDirichletBC, ScalarDoNothingBC)
from xlb_amd.operator.macroscopic import ScalarMoment
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper, ScalarTransportStepper

import _scalar_ref as ref
import _step_matrix as sm
import test_scalar_ref as pins
from _util import init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

OMEGA, OMEGA_S = 1.3, 1.45
COMBOS = [("D3Q19", "BGK", "FP32FP32"), ("D3Q27", "KBC", "FP64FP32"), ("D2Q9", "BGK", "FP64FP64")]
OTHER_AXES = ((1, 3), (2, 5), (5, 6))


def assert_same_bits(out, exp, what=""):
    assert out.dtype == exp.dtype and out.shape == exp.shape
    assert np.array_equal(out, exp), f"{what}: not bit-exact, max ulp {max_ulp_diff(out, exp)}, {int((out != exp).sum())} of {out.size} values differ"


def scalar_field(shape, seed=5):
    return np.random.default_rng(seed).uniform(0.5, 1.5, shape)


def start(stepper, f_np, phi0):
    """prepare_fields with the flow f_np and the scalar phi0"""
    return stepper.prepare_fields(scalar=phi0, initializer=lambda bc_mask, f_0: f_0.assign(f_np))


# ---- 1. passive scalar, no fluid BCs -------------------------------------------------------------------------------------------------
def passive_cases():
    out = []
    for lattice, coll, policy in COMBOS:
        k = 0
        for vec in sm.requested_vecs(policy):
            for nz in sm._nz_list(vec, "none"):
                other = OTHER_AXES[k % 3]
                k += 1
                shape = (other[0], nz) if lattice == "D2Q9" else other + (nz,)
                out.append((lattice, coll, policy, vec, shape, 3 + k % 4))
    return out


@pytest.mark.parametrize("lattice,coll,policy,vec,shape,steps", passive_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_passive_scalar_leaves_the_fluid_alone_and_matches_the_restatement(lattice, coll, policy, vec, shape, steps, exact_math):
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    ctx = get_context()
    f_np = orc.perturbed_init(shape, lat, policy, seed=11 + vec, amp_rho=0.02, amp_u=0.03)
    phi0 = scalar_field(shape)
    bm, mm = pins.no_walls(shape, lat)
    try:
        ctx.set_option("vec", vec)
        grid = grid_factory(shape)
        plain = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type=coll, backend_config={"lazy_pairs": False})
        p_0, p_1, p_bm, p_mm = plain.prepare_fields()
        p_0.assign(f_np)
        for i in range(steps):
            p_0, p_1 = plain(p_0, p_1, p_bm, p_mm, OMEGA, i)
            p_0, p_1 = p_1, p_0
        stepper = ScalarTransportStepper(grid=grid, boundary_conditions=[], collision_type=coll)
        f_0, f_1, g_0, g_1, bc_mask, missing_mask = start(stepper, f_np, phi0)
        g_np = ref.init_g(phi0, f_np, lat, policy)
        assert_same_bits(g_0.numpy(), g_np, "g_0")
        for i in range(steps):
            f_0, f_1, g_0, g_1 = stepper(f_0, f_1, g_0, g_1, bc_mask, missing_mask, OMEGA, OMEGA_S, i)
            f_0, f_1, g_0, g_1 = f_1, f_0, g_1, g_0
        assert_same_bits(f_0.numpy(), p_0.numpy(), "f against the plain stepper")
        with np.errstate(all="ignore"):
            f_e, g_e = ref.run(f_np, g_np, bm, mm, [], [], OMEGA, OMEGA_S, lat, steps, policy=policy, collision=coll)
        assert_same_bits(g_0.numpy(), g_e, "g")
        assert_same_bits(f_0.numpy(), f_e, "f against the restatement")
        phi = grid.create_field(1, dtype=stepper.precision_policy.compute_precision)
        assert_same_bits(ScalarMoment()(g_0, phi).numpy(), ref.moment(g_e, policy), "phi")
    finally:
        ctx.set_option("vec", 0)


# ---- 2. walls ------------------------------------------------------------------------------------------------------------------------
def faces(shape, remove_edges=False):
    return orc.bounding_box_indices(shape, remove_edges=remove_edges)


def union(*index_lists):
    return np.unique(np.concatenate([np.asarray(i) for i in index_lists], axis=1), axis=-1).tolist()


def heated_box(shape):
    """lid (EquilibriumBC, top) + halfway walls; Dirichlet rules on the bottom wall and the lid, the side walls adiabatic by default.
    Returns (hip BCs, hip rules, oracle BCs, restatement rules, ids whose rule must have acted)."""
    d = len(shape)
    f, f_ne = faces(shape), faces(shape, remove_edges=True)
    u_lid = (0.02, 0.0, 0.0)[:d]
    sides = union(*[f[s] for s in (["left", "right"] + (["front", "back"] if d == 3 else []))])
    lid = EquilibriumBC(rho=1.0, u=u_lid, indices=f_ne["top"])
    bottom = HalfwayBounceBackBC(indices=f_ne["bottom"])
    walls = HalfwayBounceBackBC(indices=sides)
    rules = [ScalarDirichletBC(1.0, on=bottom), ScalarDirichletBC(0.0, on=lid)]
    obcs = [orc.BC(orc.KIND_EQUILIBRIUM, lid.id, f_ne["top"], rho=1.0, u=u_lid), orc.BC(orc.KIND_HALFWAY_BB, bottom.id, f_ne["bottom"]),
            orc.BC(orc.KIND_HALFWAY_BB, walls.id, sides)]
    r_rules = [ref.Rule(ref.DIRICHLET, bottom.id, 1.0), ref.Rule(ref.DIRICHLET, lid.id, 0.0)]
    return [lid, bottom, walls], rules, obcs, r_rules, [bottom.id, lid.id, walls.id]


def channel(shape):
    """Regularized velocity inlet with a Dirichlet rule, extrapolation outflow with a do-nothing rule, fullway side walls"""
    f, f_ne = faces(shape), faces(shape, remove_edges=True)
    sides = union(*[f[s] for s in ("bottom", "top", "front", "back")])
    u_in = (0.03, 0.0, 0.0)
    walls = FullwayBounceBackBC(indices=sides)
    inlet = RegularizedBC("velocity", prescribed_value=u_in, indices=f_ne["left"])
    outlet = ExtrapolationOutflowBC(indices=f_ne["right"])
    rules = [ScalarDirichletBC(1.25, on=inlet), ScalarDoNothingBC(on=outlet), ScalarAdiabaticBC(on=walls)]
    obcs = [orc.BC(orc.KIND_FULLWAY_BB, walls.id, sides), orc.BC(orc.KIND_REGULARIZED_VELOCITY, inlet.id, f_ne["left"], prescribed=u_in),
            orc.BC(orc.KIND_EXTRAPOLATION_OUTFLOW, outlet.id, f_ne["right"])]
    r_rules = [ref.Rule(ref.DIRICHLET, inlet.id, 1.25), ref.Rule(ref.DO_NOTHING, outlet.id), ref.Rule(ref.ADIABATIC, walls.id)]
    return [walls, inlet, outlet], rules, obcs, r_rules, [inlet.id, outlet.id, walls.id]


def sphere_indices(shape):
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    inside = (x - shape[0] // 2) ** 2 + (y - shape[1] // 2) ** 2 + (z - shape[2] // 2) ** 2 < 1.6**2
    return [a.tolist() for a in np.nonzero(inside)]


def heated_sphere(shape):
    """an interior halfway sphere from indices with a Dirichlet rule in a periodic box"""
    idx = sphere_indices(shape)
    sphere = HalfwayBounceBackBC(indices=idx)
    return [sphere], [ScalarDirichletBC(1.5, on=sphere)], [orc.BC(orc.KIND_HALFWAY_BB, sphere.id, idx)], [ref.Rule(ref.DIRICHLET, sphere.id, 1.5)], [sphere.id]


WALLED = [("box", heated_box, (7, 6, 6)), ("channel", channel, (9, 6, 7)), ("sphere", heated_sphere, (8, 7, 8))]


def run_walled(build, lattice, coll, policy, shape, steps, vec=0, buoyancy=None, scalar_reference=0.0, force_vector=None):
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    ctx = get_context()
    bcs, rules, obcs, r_rules, must_act = build(shape)
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    f_np = orc.perturbed_init(shape, lat, policy, seed=23, amp_rho=0.02, amp_u=0.03)
    phi0 = scalar_field(shape, seed=7)
    try:
        ctx.set_option("vec", vec)
        stepper = ScalarTransportStepper(grid=grid_factory(shape), boundary_conditions=bcs, scalar_boundary_conditions=rules, collision_type=coll,
                                         buoyancy=buoyancy, scalar_reference=scalar_reference, force_vector=force_vector)
        f_0, f_1, g_0, g_1, bc_mask, missing_mask = start(stepper, f_np, phi0)
        assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
        f, _, g, _ = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, OMEGA, OMEGA_S, steps)
        g_np = ref.init_g(phi0, f_np, lat, policy)
        acted = {}
        with np.errstate(all="ignore"):
            f_e, g_e = ref.run(f_np, g_np, o_bm, o_mm, obcs, r_rules, OMEGA, OMEGA_S, lat, steps, policy=policy, collision=coll, acted=acted,
                               force_vector=force_vector, buoyancy=buoyancy, reference=scalar_reference)
            if buoyancy is not None:  # the coupling must matter in the case, or the comparison below shows nothing about it
                f_p, _ = ref.run(f_np, g_np, o_bm, o_mm, obcs, r_rules, OMEGA, OMEGA_S, lat, steps, policy=policy, collision=coll, force_vector=force_vector)
                assert np.abs(f_e.astype(float) - f_p).max() > 1e-5
        for bc_id in must_act:
            assert acted.get(bc_id, 0) > 0, f"the scalar rule of bc id {bc_id} acted on no cell"
        assert_same_bits(g.numpy(), g_e, "g")
        assert_same_bits(f.numpy(), f_e, "f")
    finally:
        ctx.set_option("vec", 0)


@pytest.mark.parametrize("lattice,coll,policy", [("D3Q19", "BGK", "FP32FP32"), ("D3Q27", "KBC", "FP64FP32"), ("D3Q19", "SmagorinskyLESBGK", "FP64FP64")])
@pytest.mark.parametrize("name,build,shape", WALLED, ids=[w[0] for w in WALLED])
def test_walled_cases_match_the_restatement(name, build, shape, lattice, coll, policy):
    run_walled(build, lattice, coll, policy, shape, steps=5)


@pytest.mark.parametrize("vec,nz", [(2, 6), (4, 8), (4, 6), (4, 12), (4, 4)])
def test_walled_box_with_several_cells_per_thread(vec, nz):
    # (4, 6) falls back to one cell per thread; (4, 12) has a thread at neither row end, (4, 4) one thread holding both
    run_walled(heated_box, "D3Q19", "BGK", "FP32FP32", (7, 6, nz), steps=4, vec=vec)


def test_walled_box_in_two_dimensions():
    run_walled(heated_box, "D2Q9", "BGK", "FP64FP64", (7, 8), steps=5)


def test_walled_box_with_rows_of_two_blocks_the_second_part_empty():
    # a row of 320 cells is two blocks of 192 threads (160 rounded up to whole waves); the second holds 128 cells
    run_walled(heated_box, "D2Q9", "BGK", "FP64FP64", (3, 320), steps=3)


# ---- 3. buoyancy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64"])
def test_buoyant_box_matches_the_restatement(policy):
    run_walled(heated_box, "D3Q19", "BGK", policy, (7, 6, 6), steps=5, buoyancy=np.array([0.0, 0.0, 2e-2]), scalar_reference=0.5,
               force_vector=np.array([1e-5, 0.0, 0.0]))


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64"])
def test_uniform_scalar_excess_acts_like_a_force_vector_on_the_device(policy):
    init_hip("D3Q19", policy)
    lat = orc.Lattice("D3Q19")
    shape, steps = (6, 5, 4), 5
    T = orc.compute_dtype(policy)
    buoyancy, reference, delta = np.array([0.0, 0.0, 2e-3]), 0.5, 0.25
    stepper = ScalarTransportStepper(grid=grid_factory(shape), buoyancy=buoyancy, scalar_reference=reference)
    f_0, f_1, g_0, g_1, bc_mask, missing_mask = stepper.prepare_fields(scalar=reference + delta)
    f, _, g, _ = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, 1.1, 1.3, steps)
    bm, mm = pins.no_walls(shape, lat)
    f_o = orc.run(orc.initialize_eq(shape, lat, policy), bm, mm, [], 1.1, lat, steps, policy, "BGK", force_vector=buoyancy * delta)
    rho_d, u_d = orc.macroscopic(f.numpy().astype(T), lat)
    rho_o, u_o = orc.macroscopic(f_o.astype(T), lat)
    figures = (np.abs(rho_d.astype(float) - rho_o).max(), np.abs(u_d.astype(float) - u_o).max())
    print(policy, "max |d rho| %.2e  |d u| %.2e" % figures)
    assert max(figures) <= 1e-6
    assert abs(u_d[2].astype(float).mean()) > 1e-3


# ---- 4. run(n) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5])
def test_run_equals_n_calls_and_hands_back_the_result_first(n):
    init_hip("D3Q19", "FP32FP32")
    lat = orc.Lattice("D3Q19")
    shape = (7, 6, 6)
    bcs, rules, *_ = heated_box(shape)
    f_np = orc.perturbed_init(shape, lat, "FP32FP32", seed=31, amp_rho=0.02, amp_u=0.03)
    phi0 = scalar_field(shape, seed=9)
    stepper = ScalarTransportStepper(grid=grid_factory(shape), boundary_conditions=bcs, scalar_boundary_conditions=rules, buoyancy=np.array([0.0, 0.0, 1e-3]))
    f_0, f_1, g_0, g_1, bc_mask, missing_mask = start(stepper, f_np, phi0)
    g_np = g_0.numpy()
    for i in range(n):
        f_0, f_1, g_0, g_1 = stepper(f_0, f_1, g_0, g_1, bc_mask, missing_mask, OMEGA, OMEGA_S, i)
        f_0, f_1, g_0, g_1 = f_1, f_0, g_1, g_0
    by_calls = (f_0.numpy(), g_0.numpy())
    # the same start again in the same fields (the masks are built once: the masker consumes the BCs' indices)
    r_0, r_1, h_0, h_1 = f_0.assign(f_np), f_1.fill(0.0), g_0.assign(g_np), g_1.fill(0.0)
    f, f_other, g, g_other = stepper.run(r_0, r_1, h_0, h_1, bc_mask, missing_mask, OMEGA, OMEGA_S, n)
    assert (f is r_1, g is h_1) == (n % 2 == 1, n % 2 == 1) and f_other is not f and g_other is not g
    assert_same_bits(f.numpy(), by_calls[0], "f")
    assert_same_bits(g.numpy(), by_calls[1], "g")


def test_total_scalar_in_a_periodic_box_stays_within_the_drift_of_the_cpu_pin():
    """the sine set-up of tests/test_scalar_ref.py carried by the coupled step's own uniform flow, 50 steps"""
    policy, shape, steps = "FP32FP32", (32, 4, 4), 50
    init_hip("D3Q19", policy)
    lat = orc.Lattice("D3Q19")
    T = orc.compute_dtype(policy)
    u = np.zeros((3,) + shape, T)
    u[0] = T(0.05)
    f_np = orc.equilibrium(np.ones((1,) + shape, T), u, lat, T)
    x = np.arange(shape[0]).reshape(-1, 1, 1) + 0.5
    phi0 = np.broadcast_to(1.0 + 0.1 * np.sin(2 * np.pi / shape[0] * x), shape)
    stepper = ScalarTransportStepper(grid=grid_factory(shape))
    f_0, f_1, g_0, g_1, bc_mask, missing_mask = start(stepper, f_np, phi0)
    t0 = pins.total(g_0.numpy())
    f, _, g, _ = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, 1.0, 1.25, steps)
    drift = abs(pins.total(g.numpy()) - t0) / abs(t0)
    bound = 2.0 * pins.MEASURED[("drift_periodic", 3, policy)]
    print(f"relative drift of the total scalar after {steps} steps: {drift:.3e} (bound {bound:.3e})")
    assert drift <= bound


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_at_construction():
    init_hip("D3Q19", "FP32FP32")
    shape = (8, 7, 8)
    grid = grid_factory(shape)
    f_ne = faces(shape, remove_edges=True)
    with pytest.raises(NotImplementedError, match="HybridBC"):
        ScalarTransportStepper(grid=grid, boundary_conditions=[HybridBC("bounceback_regularized", indices=sphere_indices(shape))])
    with pytest.raises(NotImplementedError, match="profile"):
        ScalarTransportStepper(grid=grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells: np.zeros_like(cells, dtype=float))])
    with pytest.raises(NotImplementedError, match="profile"):
        ScalarTransportStepper(grid=grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells, timestep: np.zeros_like(cells, dtype=float))])
    with pytest.raises(ValueError, match="[Ff]ullway"):
        fw = FullwayBounceBackBC(indices=f_ne["top"])
        ScalarTransportStepper(grid=grid, boundary_conditions=[fw], scalar_boundary_conditions=[ScalarDirichletBC(1.0, on=fw)])
    with pytest.raises(NotImplementedError, match="slab"):
        ScalarTransportStepper(grid=grid_factory(shape, backend_config={"halo": 1}))
    init_hip("D3Q19", "FP32FP16")
    with pytest.raises(NotImplementedError, match="fp16"):
        ScalarTransportStepper(grid=grid_factory(shape))


def test_the_native_layer_refuses_what_the_kernel_cannot_take():
    init_hip("D3Q19", "FP32FP32")
    shape = (4, 4, 4)
    stepper = ScalarTransportStepper(grid=grid_factory(shape))
    f_0, f_1, g_0, g_1, bc_mask, missing_mask = stepper.prepare_fields(scalar=1.0)
    before = (f_1.numpy(), g_1.numpy())
    for omega, omega_s in ((0.0, 1.0), (1.0, 2.5), (float("nan"), 1.0)):
        with pytest.raises(Exception, match="outside"):
            stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_s, 2)
    with pytest.raises(Exception, match="cardinality"):
        stepper.run(f_0, f_1, f_0, f_1, bc_mask, missing_mask, 1.0, 1.0, 1)
    with pytest.raises(_lib.HipBackendError, match="different fields"):
        _lib.Scalar.run(stepper._scalar_native(), f_0, f_1, g_0, g_0, bc_mask, missing_mask, 1.0, 1.0, 0, 1)
    assert np.array_equal(f_1.numpy(), before[0]) and np.array_equal(g_1.numpy(), before[1])  # nothing was launched
    # below the Python refusal of fp16 storage: the coupled kernels are built for three policies, and the create says so
    with pytest.raises(_lib.HipBackendError, match="built for FP32FP32, FP64FP64 and FP64FP32 only"):
        _lib.Scalar(get_context(), _lib.D3Q19, _lib.BGK, _lib.F32, _lib.F16, [])
