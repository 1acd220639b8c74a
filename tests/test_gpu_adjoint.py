"""AdjointStepper on the device against the NumPy restatement (tests/_adjoint_ref.py), bit for bit: single adjoint steps over every
lattice, policy and boundary case on small awkward shapes (periodic wrap on every axis, a row longer than one block with a ragged
tail, boundary cells on edges and corners), a checkpointed chain through ``gradient``, MacroscopicAdjoint, an end-to-end gradient
against central differences of the existing forward run, and the refusals."""

import math

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import (DoNothingBC, EquilibriumBC, ExtrapolationOutflowBC, FullwayBounceBackBC, HalfwayBounceBackBC, HybridBC,
                                                 RegularizedBC, ZouHeBC)
from xlb_amd.operator.macroscopic import Macroscopic, MacroscopicAdjoint
from xlb_amd.operator.stepper import AdjointStepper, IBMStepper, IncompressibleNavierStokesStepper, ScalarTransportStepper

import _adjoint_cases as cases
import _adjoint_ref as ref
from _util import init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

OMEGA = 1.3
POLICIES = ["FP32FP32", "FP64FP64", "FP64FP32"]
# the long axis is the contiguous one in the last entries: a row of 261 cells is two blocks with a ragged tail
SHAPES = {2: [(70, 11), (261, 5), (5, 261)], 3: [(35, 9, 6), (261, 5, 4), (4, 5, 261)]}
CASES = {"periodic": cases.periodic, "cavity-halfway": cases.cavity_halfway, "cavity-fullway": cases.cavity_fullway, "moving-wall": cases.moving_wall,
         "do-nothing": cases.do_nothing_channel}


def assert_same_bits(out, exp, what=""):
    assert out.dtype == exp.dtype and out.shape == exp.shape
    assert np.array_equal(out, exp), f"{what}: not bit-exact, max ulp {max_ulp_diff(out, exp)}, {int((out != exp).sum())} of {out.size} values differ"


def hip_bcs(obcs):
    """the HIP boundary conditions of a list of oracle descriptors, constructed in list order (ids 1, 2, ..: the descriptors' own)"""
    out = []
    for bc in obcs:
        idx = bc.indices.tolist()
        if bc.kind == orc.KIND_EQUILIBRIUM:
            hbc = EquilibriumBC(rho=bc.rho, u=tuple(bc.u), indices=idx)
        elif bc.kind == orc.KIND_HALFWAY_BB:
            hbc = HalfwayBounceBackBC(indices=idx, prescribed_value=None if bc.u_wall is None else list(bc.u_wall))
        elif bc.kind == orc.KIND_FULLWAY_BB:
            hbc = FullwayBounceBackBC(indices=idx)
        else:
            hbc = DoNothingBC(indices=idx)
        assert hbc.id == bc.id
        out.append(hbc)
    return out


def setup(case, lattice, policy, shape, seed=11):
    """(adjoint, forward stepper, fields f_0 f_1 bc_mask missing_mask, oracle side: lat, bcs, bm, mm, an off-equilibrium state)"""
    init_hip(lattice, policy)
    lat, shape, obcs = CASES[case](lattice, shape)
    grid = grid_factory(shape)
    forward = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=hip_bcs(obcs), backend_config={"lazy_pairs": False})
    f_0, f_1, bc_mask, missing_mask = forward.prepare_fields()
    bm, mm = cases.masks(shape, lat, obcs)
    assert np.array_equal(bc_mask.numpy(), bm) and np.array_equal(missing_mask.numpy(), mm.astype(np.uint8)), "masks differ"
    f_np = orc.perturbed_init(shape, lat, policy, seed=seed, amp_rho=0.02, amp_u=0.03)
    f_np = orc.step(f_np, bm, mm, obcs, OMEGA, lat, policy)
    return AdjointStepper(forward), forward, (f_0, f_1, bc_mask, missing_mask), (lat, obcs, bm, mm, f_np)


def omega_bound(terms):
    """any fixed-order fp64 sum of the same N terms is within N 2^-52 sum|t_i| of their exact sum"""
    t = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in terms])
    return math.fsum(t), t.size * 2.0**-52 * math.fsum(np.abs(t))


def single_step_cases():
    out = []
    for lattice in ("D2Q9", "D3Q19", "D3Q27"):
        for policy in POLICIES:
            for case in CASES:
                for shape in SHAPES[2 if lattice == "D2Q9" else 3]:
                    out.append((lattice, policy, case, shape))
    return out


# ---- 7. one adjoint step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,policy,case,shape", single_step_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_adjoint_step_matches_the_restatement_bit_for_bit(lattice, policy, case, shape):
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask), (lat, obcs, bm, mm, f_np) = setup(case, lattice, policy, shape)
    S = orc.store_dtype(policy)
    lam_np = np.random.default_rng(9).uniform(-1, 1, f_np.shape).astype(S)
    f_0.assign(f_np)
    lam_in, lam_out = adjoint.create_cotangent(), adjoint.create_cotangent()
    lam_in.assign(lam_np)
    adjoint.reset()
    out = adjoint.adjoint_step(f_0, lam_in, lam_out, bc_mask, missing_mask, OMEGA)
    assert out is lam_out
    exp, terms = ref.adjoint_step(f_np, lam_np, bm, mm, obcs, OMEGA, lat, policy)
    assert_same_bits(lam_out.numpy(), exp, "lam")
    assert_same_bits(lam_in.numpy(), lam_np, "lam_in must be left alone")
    d_omega = adjoint.omega_gradient()
    exact, bound = omega_bound([terms])
    assert abs(d_omega - exact) <= bound, f"dL/domega {d_omega!r} against {exact!r}: off by {abs(d_omega - exact):.3e}, bound {bound:.3e}"
    assert np.abs(exp).max() > 0.1 and exact != 0.0


# ---- 8. a chain through gradient -------------------------------------------------------------------------------------------------------
CHAIN = [("D2Q9", "FP32FP32", "cavity-halfway", (70, 11)), ("D2Q9", "FP64FP64", "do-nothing", (5, 261)), ("D2Q9", "FP64FP32", "moving-wall", (261, 5)),
         ("D3Q19", "FP32FP32", "moving-wall", (4, 5, 261)), ("D3Q19", "FP64FP64", "cavity-fullway", (35, 9, 6)), ("D3Q19", "FP64FP32", "cavity-halfway", (261, 5, 4)),
         ("D3Q27", "FP32FP32", "do-nothing", (35, 9, 6)), ("D3Q27", "FP64FP64", "periodic", (4, 5, 261)), ("D3Q27", "FP64FP32", "cavity-halfway", (35, 9, 6))]


@pytest.mark.parametrize("lattice,policy,case,shape", CHAIN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gradient_chain_with_uneven_checkpoint_segments(lattice, policy, case, shape, exact_math):
    n_steps, every = 8, 3
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask), (lat, obcs, bm, mm, f_np) = setup(case, lattice, policy, shape)
    S = orc.store_dtype(policy)
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(S)
    f_0.assign(f_np)
    states, f_final = ref.forward_states(f_np, bm, mm, obcs, OMEGA, lat, n_steps, policy)
    lam_e, terms = ref.backward(states, lam_np, bm, mm, obcs, OMEGA, lat, policy)
    exact, bound = omega_bound(terms)

    def cotangent(f):
        assert_same_bits(f.numpy(), f_final, "f_N of the forward pass")
        lam = adjoint.create_cotangent()
        lam.assign(lam_np)
        return lam

    results = []
    for _ in range(2):
        lam_0, d_omega = adjoint.gradient(f_0, bc_mask, missing_mask, OMEGA, n_steps, cotangent, checkpoint_every=every)
        assert_same_bits(lam_0.numpy(), lam_e, "lam_0")
        assert abs(d_omega - exact) <= bound, f"dL/domega {d_omega!r} against {exact!r}: off by {abs(d_omega - exact):.3e}, bound {bound:.3e}"
        results.append(d_omega)
        lam_0.free()
    assert results[0] == results[1], "dL/domega differs between two runs"
    assert_same_bits(f_0.numpy(), f_np, "f_init must be left alone")


def test_native_backward_equals_chained_single_steps():
    """the fused sweep carries mu between its steps; the public values are those of single steps chained through stored cotangents"""
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask), (lat, obcs, bm, mm, f_np) = setup("cavity-halfway", "D3Q19", "FP64FP32", (35, 9, 6))
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(np.float32)
    states_np, _ = ref.forward_states(f_np, bm, mm, obcs, OMEGA, lat, 4, "FP64FP32")
    states = []
    for s in states_np:
        states.append(adjoint.create_cotangent())
        states[-1].assign(s)
    a, b = adjoint.create_cotangent(), adjoint.create_cotangent()
    a.assign(lam_np)
    adjoint.reset()
    for s in reversed(states):
        adjoint.adjoint_step(s, a, b, bc_mask, missing_mask, OMEGA)
        a, b = b, a
    chained, d_chained = a.numpy(), adjoint.omega_gradient()
    a.assign(lam_np)
    adjoint.reset()
    lam_0, _ = adjoint.backward(states, a, b, bc_mask, missing_mask, OMEGA)
    assert_same_bits(lam_0.numpy(), chained, "sweep against chained steps")
    assert adjoint.omega_gradient() == d_chained


def test_masks_edited_in_place_between_two_sweeps():
    """AdjointStepper keeps the gathered masks of its boundary cells, keyed on the masks' addresses and contents versions (adjoint.hip):
    a sweep, both masks re-assigned IN PLACE to another variant (a solid cell of the walls' id inside the box), a second sweep through the
    same objects — both equal the restatement with the masks of their moment; a cache that kept the first variant gives the first sweep twice."""
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask), (lat, obcs, bm, mm, f_np) = setup("cavity-halfway", "D3Q19", "FP32FP32", (35, 9, 6))
    walls = obcs[1]
    obcs_2 = [obcs[0], orc.BC(walls.kind, walls.id, np.concatenate([walls.indices, [[17], [4], [3]]], axis=1))]
    bm_2, mm_2 = cases.masks((35, 9, 6), lat, obcs_2)
    assert not np.array_equal(bm, bm_2) and not np.array_equal(mm, mm_2)
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(np.float32)
    states_np, _ = ref.forward_states(f_np, bm, mm, obcs, OMEGA, lat, 3, "FP32FP32")
    states = []
    for s in states_np:
        states.append(adjoint.create_cotangent())
        states[-1].assign(s)
    a, b = adjoint.create_cotangent(), adjoint.create_cotangent()
    expected = []
    for o_bm, o_mm in ((bm, mm), (bm_2, mm_2), (bm, mm)):
        bc_mask.assign(o_bm)
        missing_mask.assign(o_mm.astype(np.uint8))
        a.assign(lam_np)
        adjoint.reset()
        lam_0, _ = adjoint.backward(states, a, b, bc_mask, missing_mask, OMEGA)
        exp, terms = ref.backward(states_np, lam_np, o_bm, o_mm, obcs, OMEGA, lat, "FP32FP32")
        assert_same_bits(lam_0.numpy(), exp, f"sweep {len(expected)}")
        exact, bound = omega_bound(terms)
        assert abs(adjoint.omega_gradient() - exact) <= bound
        expected.append(exp)
    assert not np.array_equal(expected[0], expected[1]), "the two variants give the same cotangent: the test could not tell"


def test_sweep_over_rows_of_two_blocks_the_second_part_empty():
    """(3, 320) in two dimensions: a row of 320 cells is two blocks of 192 threads (160 rounded up to whole waves), the second holding
    128 cells, and the three rows make six per-block partial sums of the omega terms per launch"""
    adjoint, forward, (f_0, f_1, bc_mask, missing_mask), (lat, obcs, bm, mm, f_np) = setup("cavity-halfway", "D2Q9", "FP64FP64", (3, 320))
    lam_np = np.random.default_rng(3).uniform(-1, 1, f_np.shape).astype(np.float64)
    states_np, _ = ref.forward_states(f_np, bm, mm, obcs, OMEGA, lat, 2, "FP64FP64")
    lam_e, terms = ref.backward(states_np, lam_np, bm, mm, obcs, OMEGA, lat, "FP64FP64")
    exact, bound = omega_bound(terms)
    states = []
    for s in states_np:
        states.append(adjoint.create_cotangent())
        states[-1].assign(s)
    a, b = adjoint.create_cotangent(), adjoint.create_cotangent()
    a.assign(lam_np)
    adjoint.reset()
    lam_0, _ = adjoint.backward(states, a, b, bc_mask, missing_mask, OMEGA)
    assert_same_bits(lam_0.numpy(), lam_e, "lam_0")
    d_omega = adjoint.omega_gradient()
    assert abs(d_omega - exact) <= bound, f"dL/domega {d_omega!r} against {exact!r}: off by {abs(d_omega - exact):.3e}, bound {bound:.3e}"
    assert np.abs(lam_e).max() > 0.1 and exact != 0.0


# ---- 9. MacroscopicAdjoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice,policy,shape", [("D2Q9", "FP64FP64", (70, 11)), ("D3Q19", "FP32FP32", (4, 5, 261)), ("D3Q27", "FP64FP32", (35, 9, 6))])
def test_macroscopic_adjoint_matches_the_restatement_bit_for_bit(lattice, policy, shape):
    vs, pp = init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    T = orc.compute_dtype(policy)
    grid = grid_factory(shape)
    f_np = orc.perturbed_init(shape, lat, policy, seed=3, amp_rho=0.02, amp_u=0.03)
    rng = np.random.default_rng(4)
    rho_bar_np, u_bar_np = rng.uniform(-1, 1, (1,) + shape).astype(T), rng.uniform(-1, 1, (lat.d,) + shape).astype(T)
    f, lam = grid.create_field(lat.q, dtype=pp.store_precision), grid.create_field(lat.q, dtype=pp.store_precision)
    rho_bar, u_bar = grid.create_field(1, dtype=pp.compute_precision), grid.create_field(lat.d, dtype=pp.compute_precision)
    f.assign(f_np)
    rho_bar.assign(rho_bar_np)
    u_bar.assign(u_bar_np)
    out = MacroscopicAdjoint()(f, rho_bar, u_bar, lam)
    assert_same_bits(out.numpy(), ref.macroscopic_adjoint(f_np, rho_bar_np, u_bar_np, lat, policy), "both cotangents")
    out = MacroscopicAdjoint()(f, None, u_bar, lam)
    assert_same_bits(out.numpy(), ref.macroscopic_adjoint(f_np, np.zeros_like(rho_bar_np), u_bar_np, lat, policy), "dL/du alone")


# ---- 10. end to end against central differences of the existing forward run -----------------------------------------------------------------
def test_gradient_of_a_velocity_loss_against_central_differences_of_the_forward_run():
    """L(omega) = 1/2 |u_N(omega) - u_target|^2 on the periodic 70 x 11 D2Q9 box in FP64FP64.  The forward ``run`` is not code under
    test; the acceptance is the convergence order of the central difference towards the adjoint gradient: the relative gap falls by
    a factor 50 .. 200 from h = 1e-3 to h = 1e-4."""
    lattice, policy, shape, n_steps, omega, omega_target = "D2Q9", "FP64FP64", (70, 11), 12, 1.3, 1.0
    vs, pp = init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    grid = grid_factory(shape)
    forward = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], backend_config={"lazy_pairs": False})
    adjoint = AdjointStepper(forward)
    f_a, f_b, bc_mask, missing_mask = forward.prepare_fields()
    f_init = grid.create_field(lat.q, dtype=pp.store_precision)
    f_init.assign(orc.perturbed_init(shape, lat, policy, seed=2, amp_rho=0.02, amp_u=0.05))
    rho, u = grid.create_field(1, dtype=pp.compute_precision), grid.create_field(lat.d, dtype=pp.compute_precision)
    macroscopic = Macroscopic()

    def velocity(om):
        f_a.copy_from(f_init)
        f, _ = forward.run(f_a, f_b, bc_mask, missing_mask, om, n_steps)
        macroscopic(f, rho, u)
        return u.numpy().astype(np.float64)

    u_target = velocity(omega_target)
    loss = lambda om: 0.5 * float(np.sum((velocity(om) - u_target) ** 2))  # noqa: E731

    def cotangent(f_final):
        macroscopic(f_final, rho, u)
        u_bar = grid.create_field(lat.d, dtype=pp.compute_precision)
        u_bar.assign(u.numpy() - u_target)
        lam = adjoint.create_cotangent()
        MacroscopicAdjoint()(f_final, None, u_bar, lam)
        return lam

    lam_0, d_omega = adjoint.gradient(f_init, bc_mask, missing_mask, omega, n_steps, cotangent, checkpoint_every=5)
    gaps = []
    for h in (1e-3, 1e-4):
        fd = (loss(omega + h) - loss(omega - h)) / (2 * h)
        gaps.append(abs(fd - d_omega) / abs(d_omega))
        print(f"h = {h:g}: central difference {fd!r}, adjoint {d_omega!r}, relative gap {gaps[-1]:.3e}")
    assert 50.0 < gaps[0] / gaps[1] < 200.0, f"gap {gaps[0]:.3e} -> {gaps[1]:.3e} is not second order"


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_at_construction():
    init_hip("D3Q19", "FP32FP32")
    shape = (8, 7, 8)
    grid = grid_factory(shape)
    f_ne = orc.bounding_box_indices(shape, remove_edges=True)
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    sphere = [a.tolist() for a in np.nonzero((x - 4) ** 2 + (y - 3) ** 2 + (z - 4) ** 2 < 1.6**2)]
    plain = lambda **kw: IncompressibleNavierStokesStepper(grid=grid, **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="SmagorinskyLESBGK"):
        AdjointStepper(plain(collision_type="SmagorinskyLESBGK"))
    with pytest.raises(NotImplementedError, match="force"):
        AdjointStepper(plain(force_vector=(1e-5, 0.0, 0.0)))
    for bc, name in ((lambda: ZouHeBC("velocity", prescribed_value=(0.02, 0.0, 0.0), indices=f_ne["left"]), "ZouHeBC"),
                     (lambda: ZouHeBC("pressure", prescribed_value=1.0, indices=f_ne["right"]), "ZouHeBC"),
                     (lambda: RegularizedBC("velocity", prescribed_value=(0.02, 0.0, 0.0), indices=f_ne["left"]), "RegularizedBC"),
                     (lambda: ExtrapolationOutflowBC(indices=f_ne["right"]), "ExtrapolationOutflowBC"),
                     (lambda: HybridBC("bounceback_regularized", indices=sphere), "HybridBC"),
                     (lambda: HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells: np.zeros_like(cells, dtype=float)), "profile"),
                     (lambda: HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells, timestep: np.zeros_like(cells, dtype=float)), "profile")):
        with pytest.raises(NotImplementedError, match=name):
            AdjointStepper(plain(boundary_conditions=[bc()]))
    with pytest.raises(NotImplementedError, match="slab"):
        AdjointStepper(IncompressibleNavierStokesStepper(grid=grid_factory(shape, backend_config={"halo": 1})))
    with pytest.raises(NotImplementedError, match="ScalarTransportStepper"):
        AdjointStepper(ScalarTransportStepper(grid=grid))
    with pytest.raises(NotImplementedError, match="IBMStepper"):
        AdjointStepper(IBMStepper(grid=grid))
    AdjointStepper(plain(boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], prescribed_value=(0.01, 0.0, 0.0))]))  # in scope
    init_hip("D3Q27", "FP32FP32")
    with pytest.raises(NotImplementedError, match="KBC"):
        AdjointStepper(IncompressibleNavierStokesStepper(grid=grid_factory(shape), collision_type="KBC"))
    for policy in ("FP32FP16", "FP64FP16"):
        init_hip("D3Q19", policy)
        with pytest.raises(NotImplementedError, match="fp16"):
            AdjointStepper(IncompressibleNavierStokesStepper(grid=grid_factory(shape)))
    # below that Python refusal: the adjoint kernels are built for three policies, and the create says so
    with pytest.raises(_lib.HipBackendError, match="built for FP32FP32, FP64FP64 and FP64FP32 only"):
        _lib.Adjoint(get_context(), _lib.D3Q19, _lib.F32, _lib.F16, [])
