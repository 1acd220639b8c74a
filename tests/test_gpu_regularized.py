"""The regularised BGK collisions (projected and recursive) on the HIP backend against the NumPy restatement tests/_regularized_ref.py:
the stepper bit for bit on odd grids (periodic; a cavity with halfway walls, an EquilibriumBC lid and one FullwayBounceBackBC face), the
stand-alone operators, the double shear layer BGK does not survive, and what is refused."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import EquilibriumBC, FullwayBounceBackBC, HalfwayBounceBackBC
from xlb_amd.operator.collision import RecursiveRegularizedBGK, RegularizedBGK
from xlb_amd.operator.equilibrium import QuadraticEquilibrium
from xlb_amd.operator.macroscopic import Macroscopic
from xlb_amd.operator.stepper import IBMStepper, IncompressibleNavierStokesStepper, ScalarTransportStepper

import _regularized_ref as ref
from _util import init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

# odd extents: rows end off a vector and off a wave boundary
SHAPES = {"D2Q9": (18, 13), "D3Q19": (13, 10, 9), "D3Q27": (13, 10, 9)}
POLICIES = ("FP32FP32", "FP64FP64", "FP64FP32")
OPERATORS = {"RegularizedBGK": RegularizedBGK, "RecursiveRegularizedBGK": RecursiveRegularizedBGK}
OMEGA, STEPS = 1.8, 20
FORCE = (1e-5, -2e-5, 3e-5)


def cavity(grid, lat):
    """[lid, floor, walls]: EquilibriumBC lid on the top face, FullwayBounceBackBC on the bottom face (both without the edges), halfway
    walls on the other faces; and the oracle's twins"""
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    sides = ["left", "right"] + (["front", "back"] if lat.d == 3 else [])
    walls = np.unique(np.array([sum((box[f][i] for f in sides), []) for i in range(lat.d)]), axis=-1).tolist()
    u_lid = (0.03,) + (0.0,) * (lat.d - 1)
    lid = EquilibriumBC(rho=1.0, u=u_lid, indices=box_ne["top"])
    floor = FullwayBounceBackBC(indices=box_ne["bottom"])
    hw = HalfwayBounceBackBC(indices=walls)
    obcs = [orc.BC(orc.KIND_EQUILIBRIUM, lid.id, box_ne["top"], rho=1.0, u=u_lid), orc.BC(orc.KIND_FULLWAY_BB, floor.id, box_ne["bottom"]),
            orc.BC(orc.KIND_HALFWAY_BB, hw.id, walls)]
    return [lid, floor, hw], obcs


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("forced", [False, True], ids=["plain", "forced"])
@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("setup", ["periodic", "cavity"])
@pytest.mark.parametrize("lattice", sorted(SHAPES))
def test_stepper_matches_the_restatement(lattice, setup, form, forced, policy):
    vs, pp = init_hip(lattice, policy)
    lat, shape = orc.Lattice(lattice), SHAPES[lattice]
    grid = grid_factory(shape)
    bcs, obcs = cavity(grid, lat) if setup == "cavity" else ([], [])
    fv = np.array(FORCE[: lat.d]) if forced else None
    f_np = ref.sheared_state(shape, lat, policy)
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    exp = ref.run(f_np, o_bm, o_mm, obcs, OMEGA, lat, form, STEPS, policy, fv)
    assert np.isfinite(exp).all()

    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs, collision_type=form, force_vector=fv)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    if bcs:
        assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
    # 20 single steps, the reference drivers' loop
    f_0.assign(f_np)
    for t in range(STEPS):
        f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, OMEGA, t)
        f_0, f_1 = f_1, f_0
    out = f_0.numpy()
    assert np.array_equal(out, exp), f"single steps: {int((out != exp).sum())} of {exp.size} values differ, max ulp {max_ulp_diff(out, exp)}"
    # ... and the same through the native run
    f_0.assign(f_np)
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, STEPS)
    out = f_0.numpy()
    assert np.array_equal(out, exp), f"run: {int((out != exp).sum())} of {exp.size} values differ, max ulp {max_ulp_diff(out, exp)}"


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64"])
@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", sorted(SHAPES))
def test_standalone_operator_matches_the_restatement(lattice, form, policy):
    vs, pp = init_hip(lattice, policy)
    lat, shape = orc.Lattice(lattice), SHAPES[lattice]
    T = orc.compute_dtype(policy)
    grid = grid_factory(shape)
    f_np = orc.stream(ref.sheared_state(shape, lat, policy).astype(T), lat)  # (streamed: off equilibrium)
    f = grid.create_field(vs.q).assign(f_np)
    rho, u = grid.create_field(1), grid.create_field(vs.d)
    Macroscopic()(f, rho, u)
    feq = QuadraticEquilibrium()(rho, u, grid.create_field(vs.q))
    out = OPERATORS[form]()(f, feq, grid.create_field(vs.q), OMEGA).numpy()
    exp = ref.collide(f_np, feq.numpy(), u.numpy(), OMEGA, lat, form)
    assert np.abs(exp - feq.numpy()).max() > 1e-6  # off equilibrium indeed
    assert np.array_equal(out, exp), max_ulp_diff(out, exp)


# ---- cells per thread x the extended boundary family (k_step's VEC and HASBC = 2) ---------------------------------------------------
@pytest.mark.parametrize("vec", [1, 2, 4])
@pytest.mark.parametrize("forced", [False, True], ids=["plain", "forced"])
@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", ["D3Q19", "D3Q27"])
def test_inlet_outlet_channel_at_every_vector_width(lattice, form, forced, vec):
    """RegularizedBC velocity inlet, ZouHeBC pressure outlet, halfway walls (the kernel variant with the Zou-He family), one, two and
    four cells per thread: nz = 12 divides by all of them, 13 x 10 rows end off a wave"""
    from xlb_amd.default_config import get_context
    from xlb_amd.operator.boundary_condition import RegularizedBC, ZouHeBC

    vs, pp = init_hip(lattice, "FP32FP32")
    lat, shape = orc.Lattice(lattice), (13, 10, 12)
    grid = grid_factory(shape)
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = np.unique(np.array([sum((box[f][i] for f in ("bottom", "top", "front", "back")), []) for i in range(3)]), axis=-1).tolist()
    u_in = (0.03, 0.0, 0.0)
    outlet = ZouHeBC("pressure", prescribed_value=1.0, indices=box_ne["right"])
    hw = HalfwayBounceBackBC(indices=walls)
    inlet = RegularizedBC("velocity", prescribed_value=u_in, indices=box_ne["left"])
    obcs = [orc.BC(orc.KIND_HALFWAY_BB, hw.id, walls), orc.BC(orc.KIND_REGULARIZED_VELOCITY, inlet.id, box_ne["left"], prescribed=u_in),
            orc.BC(orc.KIND_ZOUHE_PRESSURE, outlet.id, box_ne["right"], prescribed=1.0)]
    fv = np.array(FORCE) if forced else None
    f_np = ref.sheared_state(shape, lat, "FP32FP32", u0=0.02)
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    with np.errstate(all="ignore"):  # (the Zou-He expressions are evaluated on every cell and selected afterwards)
        exp = ref.run(f_np, o_bm, o_mm, obcs, OMEGA, lat, form, 6, "FP32FP32", fv)
    assert np.isfinite(exp).all()
    ctx = get_context()
    try:
        ctx.set_option("vec", vec)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[hw, inlet, outlet], collision_type=form, force_vector=fv)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, 6)
        out = f_0.numpy()
    finally:
        ctx.set_option("vec", 0)
    assert np.array_equal(out, exp), f"{int((out != exp).sum())} of {exp.size} values differ, max ulp {max_ulp_diff(out, exp)}"


# ---- the double shear layer of Minion and Brown at Re = 30 000 on 64 cells: BGK is lost, the regularised forms are not --------------
N, U0, RE = 64, 0.04, 30000.0
SHEAR_OMEGA = 1.0 / (3.0 * U0 * N / RE + 0.5)
SHEAR_STEPS = int(2 * N / U0)  # 3200


@pytest.fixture(scope="module")
def shear_layer_speeds():
    """max |u| after 3200 steps in FP32FP32, {(lattice, collision)}: inf when anything is not finite"""
    out = {}
    for lattice, shape in (("D2Q9", (N, N)), ("D3Q19", (N, N, 8))):
        lat = orc.Lattice(lattice)
        f_np = ref.double_shear_layer(shape, lat, "FP32FP32", U0)
        for collision in ("BGK",) + ref.FORMS:
            init_hip(lattice, "FP32FP32")
            stepper = IncompressibleNavierStokesStepper(grid=grid_factory(shape), boundary_conditions=[], collision_type=collision)
            f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
            f_0.assign(f_np)
            f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, SHEAR_OMEGA, SHEAR_STEPS)
            out[(lattice, collision)] = ref.max_speed(f_0.numpy(), lat)
            print(f"double shear layer {lattice} {collision}: max |u| = {out[(lattice, collision)]:.4f} after {SHEAR_STEPS} steps")
    return out


@pytest.mark.parametrize("lattice", ["D2Q9", "D3Q19"])
def test_double_shear_layer_survives_where_bgk_does_not(shear_layer_speeds, lattice):
    """fp64 NumPy gives 0.059-0.062 for the regularised forms; the fp32 restatement's values are in profiles/regularized_collision.md"""
    assert not shear_layer_speeds[(lattice, "BGK")] <= 0.5
    for form in ref.FORMS:
        assert shear_layer_speeds[(lattice, form)] < 0.1, (form, shear_layer_speeds[(lattice, form)])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ref.FORMS)
def test_fp16_storage_is_refused(form):
    init_hip("D3Q19", "FP32FP16")
    with pytest.raises(NotImplementedError, match=rf"collision_type '{form}': fp16 storage \(FP32FP16\) is not supported; use FP32FP32, FP64FP64 or FP64FP32"):
        IncompressibleNavierStokesStepper(grid=grid_factory((8, 8, 8)), boundary_conditions=[], collision_type=form)


@pytest.mark.parametrize("form", ref.FORMS)
def test_slab_grids_are_refused(form):
    init_hip("D3Q19")
    grid = grid_factory((8, 8, 8), backend_config={"rank": 0, "n_ranks": 2})
    with pytest.raises(NotImplementedError, match=rf"collision_type '{form}': slab-decomposed fields \(ghost planes, several ranks\) are not supported"):
        IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type=form)


@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("cls", [ScalarTransportStepper, IBMStepper])
def test_coupled_steppers_refuse_the_regularised_collisions(cls, form):
    init_hip("D3Q19")
    with pytest.raises(NotImplementedError, match=rf"{cls.__name__}: collision_type '{form}' is not supported"):
        cls(grid_factory((8, 8, 8)), [], collision_type=form)


def test_native_library_refuses_other_policies():
    """below the Python refusal: the new translation units are built for three policies, and say so as the extended collisions do"""
    from xlb_amd import _lib
    from xlb_amd.default_config import get_context

    init_hip("D3Q19", "FP32FP16")
    ctx = get_context()
    grid = grid_factory((8, 8, 8))
    f_0, f_1 = grid.create_field(19), grid.create_field(19)
    native = _lib.Stepper(ctx, _lib.D3Q19, _lib.REGULARIZED_BGK, _lib.F32, _lib.F16, [])
    with pytest.raises(RuntimeError, match="built for FP32FP32, FP64FP64 and FP64FP32 only"):
        native.step(f_0, f_1, None, None, 1.0, 0)
