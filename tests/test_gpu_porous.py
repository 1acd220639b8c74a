"""PorousStepper and its adjoint on the device against the NumPy restatement (tests/_porous_ref.py), bit for bit: forward steps and
single adjoint steps over every lattice, policy and boundary case on the adjoint suite's small awkward shapes (periodic wrap on every
axis, a row longer than one block with a ragged tail, boundary cells on edges and corners), alpha == 0 against the plain fluid stepper,
checkpointed chains through ``gradient``, an end-to-end gradient with respect to alpha against central differences of the device's
forward run, and the refusals."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import (ExtrapolationOutflowBC, HalfwayBounceBackBC, HybridBC, RegularizedBC, ZouHeBC,
                                                 boundary_condition_registry)
from xlb_amd.operator.macroscopic import Macroscopic, MacroscopicAdjoint
from xlb_amd.operator.stepper import AdjointStepper, IncompressibleNavierStokesStepper, PorousStepper

import _adjoint_cases as cases
import _porous_ref as ref
from _util import init_hip
from test_gpu_adjoint import CASES, CHAIN, OMEGA, assert_same_bits, hip_bcs, omega_bound, single_step_cases

pytestmark = pytest.mark.gpu

IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


def setup(case, lattice, policy, shape, seed=11, alpha_seed=17):
    """(adjoint, forward stepper, fields f_0 f_1 bc_mask missing_mask alpha, oracle side: lat, bcs, bm, mm, an off-equilibrium state,
    alpha seeded in [0, 0.9])"""
    init_hip(lattice, policy)
    lat, shape, obcs = CASES[case](lattice, shape)
    grid = grid_factory(shape)
    forward = PorousStepper(grid=grid, boundary_conditions=hip_bcs(obcs))
    f_0, f_1, bc_mask, missing_mask = forward.prepare_fields()
    bm, mm = cases.masks(shape, lat, obcs)
    assert np.array_equal(bc_mask.numpy(), bm) and np.array_equal(missing_mask.numpy(), mm.astype(np.uint8)), "masks differ"
    alpha_np = np.random.default_rng(alpha_seed).uniform(0.0, 0.9, (1,) + tuple(shape)).astype(orc.compute_dtype(policy))
    alpha = forward.create_solidity()
    alpha.assign(alpha_np)
    forward.set_solidity(alpha)
    f_np = orc.perturbed_init(shape, lat, policy, seed=seed, amp_rho=0.02, amp_u=0.03)
    f_np = ref.step(f_np, alpha_np, bm, mm, obcs, OMEGA, lat, policy)
    return AdjointStepper(forward), forward, (f_0, f_1, bc_mask, missing_mask, alpha), (lat, obcs, bm, mm, f_np, alpha_np)


def load_states(adjoint, states_np):
    states = []
    for s in states_np:
        states.append(adjoint.create_cotangent())
        states[-1].assign(s)
    return states


# ---- forward and single adjoint steps over the matrix ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,policy,case,shape", single_step_cases(), ids=IDS)
def test_forward_and_adjoint_step_match_the_restatement_bit_for_bit(lattice, policy, case, shape):
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask, alpha), (lat, obcs, bm, mm, f_np, alpha_np) = setup(case, lattice, policy, shape)
    S = orc.store_dtype(policy)
    # forward: one call, then two more through run
    f_0.assign(f_np)
    forward(f_0, f_1, bc_mask, missing_mask, OMEGA, 0)
    exp = ref.step(f_np, alpha_np, bm, mm, obcs, OMEGA, lat, policy)
    assert_same_bits(f_1.numpy(), exp, "one forward step")
    f, _ = forward.run(f_1, f_0, bc_mask, missing_mask, OMEGA, 2, first_timestep=1)
    assert_same_bits(f.numpy(), ref.run(exp, alpha_np, bm, mm, obcs, OMEGA, lat, 2, policy), "three forward steps")
    # one adjoint step
    lam_np = np.random.default_rng(9).uniform(-1, 1, f_np.shape).astype(S)
    f_0.assign(f_np)
    lam_in, lam_out = adjoint.create_cotangent(), adjoint.create_cotangent()
    lam_in.assign(lam_np)
    adjoint.reset()
    out = adjoint.adjoint_step(f_0, lam_in, lam_out, bc_mask, missing_mask, OMEGA)
    assert out is lam_out
    exp, terms, galpha = ref.adjoint_step(f_np, lam_np, alpha_np, bm, mm, obcs, OMEGA, lat, policy)
    assert_same_bits(lam_out.numpy(), exp, "lam")
    assert_same_bits(lam_in.numpy(), lam_np, "lam_in must be left alone")
    assert_same_bits(adjoint.solidity_gradient().numpy(), galpha.astype(np.float64)[None], "dL/dalpha")
    d_omega = adjoint.omega_gradient()
    exact, bound = omega_bound([terms])
    assert abs(d_omega - exact) <= bound, f"dL/domega {d_omega!r} against {exact!r}: off by {abs(d_omega - exact):.3e}, bound {bound:.3e}"
    assert np.abs(exp).max() > 0.1 and exact != 0.0 and np.abs(galpha).max() > 0.0


@pytest.mark.parametrize("lattice,policy,case,shape", CHAIN, ids=IDS)
def test_zero_solidity_is_the_plain_stepper_bit_for_bit(lattice, policy, case, shape, exact_math):
    lat, shape, obcs = CASES[case](lattice, shape)
    f_np = orc.perturbed_init(shape, lat, policy, seed=4, amp_rho=0.02, amp_u=0.03)
    outs = []
    for make in (lambda grid: PorousStepper(grid=grid, boundary_conditions=hip_bcs(obcs)),
                 lambda grid: IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=hip_bcs(obcs))):
        init_hip(lattice, policy)
        boundary_condition_registry.__init__()  # (the boundary conditions of either stepper get the ids 1, 2, ..: conftest.py)
        stepper = make(grid_factory(shape))
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        if isinstance(stepper, PorousStepper):
            alpha = stepper.create_solidity()
            stepper.set_solidity(alpha)
        f_0.assign(f_np)
        f, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, 5)
        outs.append(f.numpy())
    assert_same_bits(outs[0], outs[1], "alpha == 0 against the plain stepper after 5 steps")
    assert not np.array_equal(outs[0], f_np)


# ---- chains through gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,policy,case,shape", CHAIN, ids=IDS)
def test_gradient_chain_with_uneven_checkpoint_segments(lattice, policy, case, shape):
    n_steps, every = 8, 3
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask, alpha), (lat, obcs, bm, mm, f_np, alpha_np) = setup(case, lattice, policy, shape)
    S = orc.store_dtype(policy)
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(S)
    f_0.assign(f_np)
    states, f_final = ref.forward_states(f_np, alpha_np, bm, mm, obcs, OMEGA, lat, n_steps, policy)
    lam_e, terms, dalpha_e = ref.backward(states, lam_np, alpha_np, bm, mm, obcs, OMEGA, lat, policy)
    exact, bound = omega_bound(terms)

    def cotangent(f):
        assert_same_bits(f.numpy(), f_final, "f_N of the forward pass")
        lam = adjoint.create_cotangent()
        lam.assign(lam_np)
        return lam

    results = []
    for _ in range(2):
        lam_0, d_omega, d_alpha = adjoint.gradient(f_0, bc_mask, missing_mask, OMEGA, n_steps, cotangent, checkpoint_every=every)
        assert_same_bits(lam_0.numpy(), lam_e, "lam_0")
        assert d_alpha.dtype == np.float64
        assert_same_bits(d_alpha.numpy(), dalpha_e, "dL/dalpha")
        assert abs(d_omega - exact) <= bound, f"dL/domega {d_omega!r} against {exact!r}: off by {abs(d_omega - exact):.3e}, bound {bound:.3e}"
        results.append((d_omega, d_alpha.numpy()))
        lam_0.free()
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1]), "the gradients differ between two runs"
    assert_same_bits(f_0.numpy(), f_np, "f_init must be left alone")
    assert np.abs(dalpha_e).max() > 0.0
    adjoint.reset()
    assert not adjoint.solidity_gradient().numpy().any() and adjoint.omega_gradient() == 0.0


def test_native_backward_equals_chained_single_steps():
    """the fused sweep carries mu between its steps; the public values are those of single steps chained through stored cotangents"""
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask, alpha), (lat, obcs, bm, mm, f_np, alpha_np) = setup("cavity-halfway", "D3Q19", "FP64FP32", (35, 9, 6))
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(np.float32)
    states_np, _ = ref.forward_states(f_np, alpha_np, bm, mm, obcs, OMEGA, lat, 4, "FP64FP32")
    states = load_states(adjoint, states_np)
    a, b = adjoint.create_cotangent(), adjoint.create_cotangent()
    a.assign(lam_np)
    adjoint.reset()
    for s in reversed(states):
        adjoint.adjoint_step(s, a, b, bc_mask, missing_mask, OMEGA)
        a, b = b, a
    chained, d_chained, g_chained = a.numpy(), adjoint.omega_gradient(), adjoint.solidity_gradient().numpy()
    a.assign(lam_np)
    adjoint.reset()
    lam_0, _ = adjoint.backward(states, a, b, bc_mask, missing_mask, OMEGA)
    assert_same_bits(lam_0.numpy(), chained, "sweep against chained steps")
    assert adjoint.omega_gradient() == d_chained
    assert_same_bits(adjoint.solidity_gradient().numpy(), g_chained, "dL/dalpha of the sweep against chained steps")
    assert np.abs(g_chained).max() > 0.0


def test_sweep_over_rows_of_two_blocks_the_second_part_empty():
    """(3, 320) in two dimensions: a row of 320 cells is two blocks of 192 threads (160 rounded up to whole waves), the second holding
    128 cells: its idle threads must neither store populations nor touch the gradient field"""
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask, alpha), (lat, obcs, bm, mm, f_np, alpha_np) = setup("cavity-halfway", "D2Q9", "FP64FP64", (3, 320))
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(np.float64)
    f_0.assign(f_np)
    f, _ = forward.run(f_0, f_1, bc_mask, missing_mask, OMEGA, 2)
    states_np, f_final = ref.forward_states(f_np, alpha_np, bm, mm, obcs, OMEGA, lat, 2, "FP64FP64")
    assert_same_bits(f.numpy(), f_final, "two forward steps")
    lam_e, terms, dalpha_e = ref.backward(states_np, lam_np, alpha_np, bm, mm, obcs, OMEGA, lat, "FP64FP64")
    exact, bound = omega_bound(terms)
    states = load_states(adjoint, states_np)
    a, b = adjoint.create_cotangent(), adjoint.create_cotangent()
    a.assign(lam_np)
    adjoint.reset()
    lam_0, _ = adjoint.backward(states, a, b, bc_mask, missing_mask, OMEGA)
    assert_same_bits(lam_0.numpy(), lam_e, "lam_0")
    assert_same_bits(adjoint.solidity_gradient().numpy(), dalpha_e, "dL/dalpha")
    d_omega = adjoint.omega_gradient()
    assert abs(d_omega - exact) <= bound, f"dL/domega {d_omega!r} against {exact!r}: off by {abs(d_omega - exact):.3e}, bound {bound:.3e}"
    assert np.abs(lam_e).max() > 0.1 and exact != 0.0


# ---- end to end against central differences of the device's forward run ------------------------------------------------------------------
def test_gradient_of_a_velocity_loss_with_respect_to_alpha_against_central_differences():
    """L(alpha) = 1/2 |u_N(alpha) - u_target|^2 on the periodic (8, 7, 8) D3Q19 box in FP64FP64, along one seeded direction of alpha.
    The acceptance is the convergence order of the central difference of the device's forward ``run`` towards the adjoint gradient:
    the relative gap falls by a factor 50 .. 200 from h = 1e-3 to h = 1e-4 (test_gpu_adjoint.py's bound for its end-to-end case)."""
    lattice, policy, shape, n_steps, omega = "D3Q19", "FP64FP64", (8, 7, 8), 12, 1.3
    vs, pp = init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    grid = grid_factory(shape)
    forward = PorousStepper(grid=grid, boundary_conditions=[])
    adjoint = AdjointStepper(forward)
    f_a, f_b, bc_mask, missing_mask = forward.prepare_fields()
    f_init = grid.create_field(lat.q, dtype=pp.store_precision)
    f_init.assign(orc.perturbed_init(shape, lat, policy, seed=2, amp_rho=0.02, amp_u=0.05))
    rho, u = grid.create_field(1, dtype=pp.compute_precision), grid.create_field(lat.d, dtype=pp.compute_precision)
    macroscopic = Macroscopic()
    rng = np.random.default_rng(31)
    alpha_np, alpha_target, da = rng.uniform(0.0, 0.9, (1,) + shape), rng.uniform(0.0, 0.9, (1,) + shape), rng.uniform(-1, 1, (1,) + shape)
    alpha = forward.create_solidity()
    forward.set_solidity(alpha)

    def velocity(a):
        alpha.assign(a)
        f_a.copy_from(f_init)
        f, _ = forward.run(f_a, f_b, bc_mask, missing_mask, omega, n_steps)
        macroscopic(f, rho, u)
        return u.numpy().astype(np.float64)

    u_target = velocity(alpha_target)
    loss = lambda a: 0.5 * float(np.sum((velocity(a) - u_target) ** 2))  # noqa: E731

    def cotangent(f_final):
        macroscopic(f_final, rho, u)
        u_bar = grid.create_field(lat.d, dtype=pp.compute_precision)
        u_bar.assign(u.numpy() - u_target)
        lam = adjoint.create_cotangent()
        MacroscopicAdjoint()(f_final, None, u_bar, lam)
        return lam

    alpha.assign(alpha_np)
    lam_0, d_omega, d_alpha = adjoint.gradient(f_init, bc_mask, missing_mask, omega, n_steps, cotangent, checkpoint_every=5)
    directional = float(np.sum(d_alpha.numpy() * da))
    gaps = []
    for h in (1e-3, 1e-4):
        fd = (loss(alpha_np + h * da) - loss(alpha_np - h * da)) / (2 * h)
        gaps.append(abs(fd - directional) / abs(directional))
        print(f"h = {h:g}: central difference {fd!r}, adjoint {directional!r}, relative gap {gaps[-1]:.3e}")
    assert 50.0 < gaps[0] / gaps[1] < 200.0, f"gap {gaps[0]:.3e} -> {gaps[1]:.3e} is not second order"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    init_hip("D3Q19", "FP32FP32")
    shape = (8, 7, 8)
    grid = grid_factory(shape)
    f_ne = orc.bounding_box_indices(shape, remove_edges=True)
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sphere = [a.tolist() for a in np.nonzero((x - 4) ** 2 + (y - 3) ** 2 + (z - 4) ** 2 < 1.6**2)]
    for collision in ("SmagorinskyLESBGK", "KBC", "RegularizedBGK", "RecursiveRegularizedBGK"):
        with pytest.raises(NotImplementedError, match=collision):
            PorousStepper(grid=grid, collision_type=collision)
    with pytest.raises(TypeError, match="force_vector"):
        PorousStepper(grid=grid, force_vector=(1e-5, 0.0, 0.0))
    for bc, name in ((lambda: ZouHeBC("velocity", prescribed_value=(0.02, 0.0, 0.0), indices=f_ne["left"]), "ZouHeBC"),
                     (lambda: ZouHeBC("pressure", prescribed_value=1.0, indices=f_ne["right"]), "ZouHeBC"),
                     (lambda: RegularizedBC("velocity", prescribed_value=(0.02, 0.0, 0.0), indices=f_ne["left"]), "RegularizedBC"),
                     (lambda: ExtrapolationOutflowBC(indices=f_ne["right"]), "ExtrapolationOutflowBC"),
                     (lambda: HybridBC("bounceback_regularized", indices=sphere), "HybridBC"),
                     (lambda: HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells: np.zeros_like(cells, dtype=float)), "profile"),
                     (lambda: HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells, timestep: np.zeros_like(cells, dtype=float)), "profile")):
        with pytest.raises(NotImplementedError, match=name):
            PorousStepper(grid=grid, boundary_conditions=[bc()])
    with pytest.raises(NotImplementedError, match="slab"):
        PorousStepper(grid=grid_factory(shape, backend_config={"halo": 1}))
    # in scope: a constant wall velocity; and the solidity field's checks
    stepper = PorousStepper(grid=grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], prescribed_value=(0.01, 0.0, 0.0))])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    with pytest.raises(Exception, match="no solidity field is bound"):  # (Operator.__call__ wraps what its implementation raises)
        stepper(f_0, f_1, bc_mask, missing_mask, OMEGA, 0)
    with pytest.raises(RuntimeError, match="set_solidity"):
        stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, 2)
    with pytest.raises(RuntimeError, match="set_solidity"):
        AdjointStepper(stepper).reset()
    from xlb_amd.precision_policy import Precision

    with pytest.raises(ValueError, match="compute dtype"):
        stepper.set_solidity(grid.create_field(1, dtype=Precision.FP64))
    with pytest.raises(ValueError, match="shape"):
        stepper.set_solidity(grid.create_field(3, dtype=Precision.FP32))
    with pytest.raises(ValueError, match="shape"):
        stepper.set_solidity(grid_factory((8, 7, 9)).create_field(1, dtype=Precision.FP32))
    with pytest.raises(TypeError):
        stepper.set_solidity(np.zeros((1,) + shape, np.float32))
    with pytest.raises(NotImplementedError, match="not a PorousStepper"):
        AdjointStepper(IncompressibleNavierStokesStepper(grid=grid)).solidity_gradient()
    stepper.set_solidity(stepper.create_solidity(0.25))
    stepper(f_0, f_1, bc_mask, missing_mask, OMEGA, 0)
    # natively: the step before a binding, a solidity field of the wrong dtype or grid
    native = _lib.Porous(get_context(), _lib.D3Q19, _lib.F32, _lib.F32, [])
    with pytest.raises(_lib.HipBackendError, match="no solidity field is bound"):
        native.step(f_0, f_1, None, None, OMEGA, 0)
    with pytest.raises(_lib.HipBackendError, match="compute dtype"):
        native.set_solidity(grid.create_field(1, dtype=Precision.FP64))
    native.set_solidity(grid_factory((8, 7, 9)).create_field(1, dtype=Precision.FP32))
    with pytest.raises(_lib.HipBackendError, match="solidity field is on a"):
        native.step(f_0, f_1, None, None, OMEGA, 0)
    for policy in ("FP32FP16", "FP64FP16"):
        init_hip("D3Q19", policy)
        with pytest.raises(NotImplementedError, match="fp16"):
            PorousStepper(grid=grid_factory(shape))
    # below that Python refusal: the porous kernels are built for three policies, and the create says so
    with pytest.raises(_lib.HipBackendError, match="built for FP32FP32, FP64FP64 and FP64FP32 only"):
        _lib.Porous(get_context(), _lib.D3Q19, _lib.F32, _lib.F16, [])


def test_rebinding_on_another_grid_of_as_many_cells_starts_a_new_gradient():
    """the gradient field belongs to the solidity's grid (nx, ny, nz), not to its number of cells"""
    vs, pp = init_hip("D3Q19", "FP64FP64")
    from xlb_amd.precision_policy import Precision

    lat = orc.Lattice("D3Q19")
    grid_a, grid_b = grid_factory((8, 7, 8)), grid_factory((8, 8, 7))
    native = _lib.Porous(get_context(), _lib.D3Q19, _lib.F64, _lib.F64, [])
    alpha_a, alpha_b = grid_a.create_field(1, dtype=Precision.FP64, fill_value=0.3), grid_b.create_field(1, dtype=Precision.FP64, fill_value=0.3)
    f, lam, out = (grid_a.create_field(lat.q, dtype=Precision.FP64) for _ in range(3))
    f.assign(orc.perturbed_init((8, 7, 8), lat, "FP64FP64", seed=2, amp_rho=0.02, amp_u=0.05))
    lam.assign(np.random.default_rng(1).uniform(-1, 1, f.shape))
    native.set_solidity(alpha_a)
    native.adjoint_step(f, lam, out, None, None, OMEGA)
    g_a = native.solidity_gradient(grid_a.create_field(1, dtype=Precision.FP64)).numpy()
    assert np.abs(g_a).max() > 0.0
    native.set_solidity(alpha_a)  # the same grid: the gradient stays
    assert np.array_equal(native.solidity_gradient(grid_a.create_field(1, dtype=Precision.FP64)).numpy(), g_a)
    native.set_solidity(alpha_b)
    assert not native.solidity_gradient(grid_b.create_field(1, dtype=Precision.FP64)).numpy().any()
    with pytest.raises(_lib.HipBackendError, match="solidity"):
        native.solidity_gradient(grid_a.create_field(1, dtype=Precision.FP64))
