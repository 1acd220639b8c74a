"""Time-dependent wall velocities: HalfwayBounceBackBC / HybridBC with ``profile(cells, timestep)`` (the reference's kernel backends:
bc_halfway_bounce_back.py:147-155, bc_hybrid.py:163-172 and :228-239; the stepper passes its timestep to every BC functional,
nse_stepper.py:370-378).  The expected fields come from oracle/mesh_bc.step called once per step with the wall velocity the profile
gives at that step's t; the step from f(t) to f(t+1) uses profile(cells, t)."""

import numpy as np
import pytest

from oracle import mesh_bc as mb
from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC, HybridBC, ZouHeBC
from xlb_amd.operator.boundary_masker import BC_SOLID, MeshVoxelizationMethod
from xlb_amd.operator.force import MomentumTransfer
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

from _util import cavity_indices, icosphere, init_hip

pytestmark = pytest.mark.gpu
KINDS = {"bounceback_regularized": mb.KIND_HYBRID_BB_REGULARIZED, "bounceback_grads": mb.KIND_HYBRID_BB_GRADS,
         "nonequilibrium_regularized": mb.KIND_HYBRID_NEQ_REGULARIZED}


def all_cells(shape):
    return np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")).reshape(len(shape), -1)


def wall_field(profile, shape, t):
    """the profile at t on every cell, (d,) + shape: the oracle's per-cell u_wall (only the BC's cells matter)"""
    return np.asarray(profile(all_cells(shape), t), np.float64).reshape((len(shape),) + tuple(shape))


def oracle_run(f_np, o_bm, o_mm, bcs_at, omega, lat, t0, n, policy="FP32FP32", collision="BGK"):
    """n oracle steps from timestep t0; bcs_at(t) is the BC list of the step from f(t) to f(t+1)"""
    f = f_np
    with np.errstate(all="ignore"):
        for t in range(t0, t0 + n):
            f = mb.step(f, o_bm, o_mm, bcs_at(t), omega, lat, policy, collision)
    return f


def ref_loop(stepper, f_0, f_1, bc_mask, missing_mask, omega, t0, n):
    """the reference's driver loop (nse_stepper.py docstring): stepper(..., i) and swap"""
    for t in range(t0, t0 + n):
        f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, omega, t)
        f_0, f_1 = f_1, f_0
    return f_0, f_1


def ramp_lid(nx, d, u0=0.05, ramp=6):
    """u(x, t) = U(x) min(1, (t + 1) / T) along the first axis: a lid driven from rest, fastest in its middle"""

    def profile(cells, t):
        u = u0 * np.sin(np.pi * (cells[0].astype(np.float64) + 0.5) / nx) * min(1.0, (t + 1) / ramp)
        return np.stack([u] + [np.zeros_like(u)] * (d - 1))

    return profile


def cavity(lattice, shape, profile):
    vs, pp = init_hip(lattice)
    lat = orc.Lattice(lattice)
    grid = grid_factory(shape)
    lid, walls = cavity_indices(grid, lat.d)
    bc_lid = HalfwayBounceBackBC(profile=profile, indices=lid)
    bc_walls = HalfwayBounceBackBC(indices=walls)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[bc_lid, bc_walls])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    o_w = orc.BC(orc.KIND_HALFWAY_BB, bc_walls.id, walls)
    o_bm, o_mm = orc.build_masks(shape, lat, [orc.BC(orc.KIND_HALFWAY_BB, bc_lid.id, lid), o_w])
    assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
    return lat, stepper, bc_lid, (f_0, f_1, bc_mask, missing_mask), (o_bm, o_mm, o_w)


@pytest.mark.parametrize("lattice,shape", [("D2Q9", (20, 16)), ("D3Q19", (12, 10, 14))])
def test_ramped_lid_vs_oracle(lattice, shape):
    """A spatially varying lid ramped up from rest: run() from first_timestep != 0 with an odd count, and the reference-style loop,
    agree with each other and with the oracle bit for bit; the same run with the lid frozen at t0 differs."""
    profile = ramp_lid(shape[0], len(shape))
    lat, stepper, bc_lid, (f_0, f_1, bc_mask, missing_mask), (o_bm, o_mm, o_w) = cavity(lattice, shape, profile)
    assert bc_lid.is_time_dependent
    f_np = orc.perturbed_init(shape, lat, seed=61, amp_rho=0.01, amp_u=0.02)
    t0, n, omega = 3, 7, 1.4
    f_0.assign(f_np)
    a, b = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=t0)
    out_run = a.numpy()
    a.assign(f_np)
    c, _ = ref_loop(stepper, a, b, bc_mask, missing_mask, omega, t0, n)
    out_loop = c.numpy()
    exp = oracle_run(f_np, o_bm, o_mm, lambda t: [mb.HalfwayProfileBC(bc_lid.id, None, wall_field(profile, shape, t)), o_w], omega, lat, t0, n)
    assert np.isfinite(out_run).all()
    assert np.array_equal(out_run, out_loop)
    assert np.array_equal(out_run, exp)
    frozen = oracle_run(f_np, o_bm, o_mm, lambda t: [mb.HalfwayProfileBC(bc_lid.id, None, wall_field(profile, shape, t0)), o_w], omega, lat, t0, n)
    assert not np.array_equal(frozen, exp)  # time really passes


def end_plane_case(plate, shape=(24, 16, 64)):
    """halfway walls on the y / z faces, a time-dependent wall on the plane x = 0 and a static one on x = nx - 1: the two-step kernel
    takes it (fuse2 = 2) with the end planes through the single-step kernel (stepper.hip: step_twice_edge_ext)"""
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    grid = grid_factory(shape)
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [sum((box[f][i] for f in ("bottom", "top", "front", "back")), []) for i in range(3)]
    walls = np.unique(np.array(walls), axis=-1).tolist()
    b_w = HalfwayBounceBackBC(indices=walls)
    b_p = HalfwayBounceBackBC(profile=plate, indices=box_ne["left"])
    b_r = HalfwayBounceBackBC(indices=box_ne["right"])
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[b_w, b_p, b_r])
    fields = stepper.prepare_fields()
    o_w, o_r = orc.BC(orc.KIND_HALFWAY_BB, b_w.id, walls), orc.BC(orc.KIND_HALFWAY_BB, b_r.id, box_ne["right"])
    o_bm, o_mm = orc.build_masks(shape, lat, [o_w, orc.BC(orc.KIND_HALFWAY_BB, b_p.id, box_ne["left"]), o_r])
    assert np.array_equal(fields[2].numpy(), o_bm) and np.array_equal(fields[3].numpy(), o_mm.astype(np.uint8))

    def bcs_at(t):
        return [o_w, mb.HalfwayProfileBC(b_p.id, None, wall_field(plate, shape, t)), o_r]

    return lat, stepper, fields, (o_bm, o_mm, bcs_at)


def oscillating_plate(cells, t):
    y = cells[1].astype(np.float64)
    s = np.sin(2.0 * np.pi * t / 6.0)
    return np.stack([np.zeros_like(y), 0.01 * s * np.ones_like(y), 0.03 * s * (1.0 + 0.5 * np.cos(y))])


def test_time_dependent_wall_on_an_x_end_plane_fused_pairs():
    """The fused pair's end planes read table t in their first single step and t + 1 in their second: run() with even and odd counts,
    the reference-style loop (pairs fused, the virtual field read once mid-run) — all bit-exact against the oracle."""
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        lat, stepper, (f_0, f_1, bc_mask, missing_mask), (o_bm, o_mm, bcs_at) = end_plane_case(oscillating_plate)
        shape = f_0.grid_shape
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_np = orc.perturbed_init(shape, lat, seed=67, amp_rho=0.01, amp_u=0.02)
        omega = 1.5
        for t0, n in ((0, 6), (5, 7)):
            f_0.assign(f_np)
            a, b = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=t0)
            exp = oracle_run(f_np, o_bm, o_mm, bcs_at, omega, lat, t0, n)
            assert np.array_equal(a.numpy(), exp), (t0, n)
            f_0, f_1 = a, b
        # reference-style loop: pairs (t, t + 1) fused, the field holding f(t + 1) virtually read once
        t0, n = 2, 9
        f_0.assign(f_np)
        pairs0, mat0 = stepper._n_fused_pairs, stepper._n_materialised
        c, d = f_0, f_1
        mid = None
        for i, t in enumerate(range(t0, t0 + n)):
            c, d = stepper(c, d, bc_mask, missing_mask, omega, t)
            c, d = d, c
            if i == 3:
                mid = d.numpy()  # f(t0 + 3), left virtual by the pair (t0 + 2, t0 + 3)
        out = c.numpy()
        assert stepper._n_fused_pairs > pairs0 and stepper._n_materialised > mat0
        assert np.array_equal(mid, oracle_run(f_np, o_bm, o_mm, bcs_at, omega, lat, t0, 3))
        assert np.array_equal(out, oracle_run(f_np, o_bm, o_mm, bcs_at, omega, lat, t0, n))
    finally:
        ctx.set_option("fuse2", 1)


@pytest.mark.parametrize("bc_method", list(KINDS))
@pytest.mark.parametrize("with_dist", [False, True])
@pytest.mark.parametrize("lattice,policy", [("D3Q19", "FP32FP32"), ("D3Q27", "FP64FP32")])
def test_hybrid_bc_rotation_rate_changing_in_time_vs_oracle(bc_method, with_dist, lattice, policy, exact_math):
    """A RAY-voxelised mesh sphere whose rotation rate is omega(t) = omega0 sin(2 pi t / P): HybridBC(profile=f(cells, t)), 6 steps from
    t = 1 against the oracle, fluid cells bit for bit."""
    shape, center, radius = (18, 16, 14), (8.3, 7.6, 6.9), 3.7
    vs, pp = init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    grid = grid_factory(shape)
    verts = icosphere(center, radius, 1)
    w0 = np.array([0.0, 0.006, -0.003])

    def profile(cells, t):
        rot = w0 * np.sin(2.0 * np.pi * t / 8.0)
        return np.cross(rot.reshape(1, 3), (cells.astype(np.float64) - np.asarray(center).reshape(3, 1)).T).T

    b_s = HybridBC(bc_method, profile=profile, mesh_vertices=verts, voxelization_method=MeshVoxelizationMethod("RAY"), use_mesh_distance=with_dist)
    collision = "KBC" if lattice == "D3Q27" else "BGK"
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[b_s], collision_type=collision)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    z1, zq = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    res = mb.mesh_mask_ray(shape, lat, b_s.id, verts, z1, zq, np.zeros((lat.q,) + shape, np.float32) if with_dist else None)
    o_bm, o_mm, o_d = res[0], res[1], (res[2] if with_dist else None)
    assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
    f_np = orc.perturbed_init(shape, lat, policy, seed=71, amp_rho=0.01, amp_u=0.02)
    f_0.assign(f_np)
    t0, n, omega = 1, 6, 1.4
    a, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=t0)
    out = a.numpy()
    exp = oracle_run(f_np, o_bm, o_mm, lambda t: [mb.HybridBC(KINDS[bc_method], b_s.id, None, u_wall=wall_field(profile, shape, t), distances=o_d)],
                     omega, lat, t0, n, policy, collision)
    fluid = np.broadcast_to(o_bm != BC_SOLID, out.shape)
    assert np.isfinite(out[fluid]).all()
    assert np.array_equal(out[fluid], exp[fluid])


@pytest.mark.parametrize("case", ["d2q9_single_steps", "d3q19_fused_pairs"])
def test_more_steps_than_the_ring_holds(case):
    """Runs several times longer than the ring of per-timestep tables, with an odd total: chunked staging, identical to the oracle."""
    if case == "d2q9_single_steps":
        shape = (10, 8)
        profile = ramp_lid(shape[0], 2, ramp=1000)  # (longer than the run: every step's table differs from its neighbours')
        lat, stepper, bc_lid, (f_0, f_1, bc_mask, missing_mask), (o_bm, o_mm, o_w) = cavity("D2Q9", shape, profile)

        def bcs_at(t):
            return [mb.HalfwayProfileBC(bc_lid.id, None, wall_field(profile, shape, t)), o_w]

        ctx = None
    else:
        ctx = get_context()
        ctx.set_option("fuse2", 2)
        lat, stepper, (f_0, f_1, bc_mask, missing_mask), (o_bm, o_mm, bcs_at) = end_plane_case(oscillating_plate)
        shape = f_0.grid_shape
    try:
        slots = stepper._native_stepper().profile_slots()
        assert slots >= 4 and slots % 2 == 0
        n, t0 = 2 * slots + 7, 11
        f_np = orc.perturbed_init(shape, lat, seed=73, amp_rho=0.01, amp_u=0.02)
        f_0.assign(f_np)
        a, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.3, n, first_timestep=t0)
        assert np.array_equal(a.numpy(), oracle_run(f_np, o_bm, o_mm, bcs_at, 1.3, lat, t0, n))
    finally:
        if ctx is not None:
            ctx.set_option("fuse2", 1)


def test_mixed_static_and_time_dependent_tables():
    """A Zou-He inlet with a time-independent profile() and a time-dependent halfway wall share one table: the static entries stay in
    every staged image."""
    shape = (16, 8, 12)
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    grid = grid_factory(shape)
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [sum((box[f][i] for f in ("bottom", "top", "front", "back")), []) for i in range(3)]
    walls = np.unique(np.array(walls), axis=-1).tolist()
    y, z = np.meshgrid(np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    prof = np.zeros((3, shape[1], shape[2]))
    prof[0] = 0.03 * np.maximum(0.0, 1.0 - ((2.0 * y / (shape[1] - 1) - 1.0) ** 2 + (2.0 * z / (shape[2] - 1) - 1.0) ** 2))
    x, yy, zz = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    body = [s.tolist() for s in np.where((x - 7) ** 2 + (yy - 4) ** 2 + (zz - 6) ** 2 < 2.2**2)]
    ctr = np.array([7.0, 4.0, 6.0]).reshape(3, 1)

    def spin(cells, t):
        return np.cross(np.array([[0.0, 0.0, 0.004 * (1 + t % 3)]]), (cells.astype(np.float64) - ctr).T).T

    b_w = HalfwayBounceBackBC(indices=walls)
    b_in = ZouHeBC("velocity", profile=lambda: prof, indices=box_ne["left"])
    b_out = ZouHeBC("pressure", prescribed_value=1.0, indices=box_ne["right"])
    b_s = HalfwayBounceBackBC(profile=spin, indices=body)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[b_w, b_in, b_out, b_s])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    o_w = orc.BC(orc.KIND_HALFWAY_BB, b_w.id, walls)
    o_in = orc.BC(orc.KIND_ZOUHE_VELOCITY, b_in.id, box_ne["left"], prescribed=prof)
    o_out = orc.BC(orc.KIND_ZOUHE_PRESSURE, b_out.id, box_ne["right"], prescribed=1.0)
    o_bm, o_mm = orc.build_masks(shape, lat, [o_w, o_in, o_out, orc.BC(orc.KIND_HALFWAY_BB, b_s.id, body)])
    assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
    f_np = orc.perturbed_init(shape, lat, seed=79, amp_rho=0.01, amp_u=0.02)
    f_0.assign(f_np)
    t0, n = 4, 9
    a, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.2, n, first_timestep=t0)
    exp = oracle_run(f_np, o_bm, o_mm, lambda t: [o_w, o_in, o_out, mb.HalfwayProfileBC(b_s.id, None, wall_field(spin, shape, t))], 1.2, lat, t0, n)
    assert np.array_equal(a.numpy(), exp)


def test_two_argument_profile_that_ignores_time_gives_the_static_bits():
    shape = (12, 10, 14)
    lid_u = ramp_lid(shape[0], 3, ramp=1)  # min(1, (t + 1) / 1) = 1 for every t >= 0

    outs = []
    for profile in (lambda cells: lid_u(cells, 0), lambda cells, t: lid_u(cells, 0)):
        lat, stepper, bc_lid, (f_0, f_1, bc_mask, missing_mask), _ = cavity("D3Q19", shape, profile)
        assert bc_lid.is_time_dependent == (profile.__code__.co_argcount == 2)
        f_0.assign(orc.perturbed_init(shape, lat, seed=83, amp_rho=0.01, amp_u=0.02))
        a, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 7, first_timestep=2)
        outs.append(a.numpy())
    assert np.array_equal(outs[0], outs[1])


def test_momentum_transfer_on_a_time_dependent_wall():
    """MomentumTransfer(bc) evaluates the wall at timestep 0 by default (the reference's momentum_transfer.py:88); timestep=t asks for
    the wall velocity at t.  Both against the oracle's force, with the tolerances of test_halfway_bc_wall_velocity_profile_vs_oracle."""
    shape, center, radius = (18, 16, 14), (8.3, 7.6, 6.9), 3.7
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    grid = grid_factory(shape)
    w0, ctr = np.array([0.003, 0.0, -0.004]), np.asarray(center).reshape(3, 1)

    def profile(cells, t):
        return np.cross((w0 * min(1.0, (t + 1) / 8.0)).reshape(1, 3), (cells.astype(np.float64) - ctr).T).T

    verts = icosphere(center, radius, 1)
    bc = HalfwayBounceBackBC(profile=profile, mesh_vertices=verts, voxelization_method=MeshVoxelizationMethod("RAY"))
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[bc])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    z1, zq = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    o_bm, o_mm = mb.mesh_mask_ray(shape, lat, bc.id, verts, z1, zq, None)[:2]
    f_np = orc.perturbed_init(shape, lat, seed=89, amp_rho=0.01, amp_u=0.02)
    f_0.assign(f_np)
    n = 9
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, n)
    out = f_0.numpy()
    exp = oracle_run(f_np, o_bm, o_mm, lambda t: [mb.HalfwayProfileBC(bc.id, None, wall_field(profile, shape, t))], 1.5, lat, 0, n)
    fluid = np.broadcast_to(o_bm != BC_SOLID, out.shape)
    assert np.array_equal(out[fluid], exp[fluid])
    f_fluid = np.where(fluid, out, 0).astype(out.dtype)
    forces = {}
    for t in (None, 0, 7):
        force = MomentumTransfer(bc)(f_0, f_1, bc_mask, missing_mask) if t is None else MomentumTransfer(bc)(f_0, f_1, bc_mask, missing_mask, timestep=t)
        with np.errstate(all="ignore"):
            fexp = mb.momentum_transfer(f_fluid, mb.HalfwayProfileBC(bc.id, None, wall_field(profile, shape, t or 0)), o_bm, o_mm, lat)
        assert force.shape == (3,) and np.allclose(force, fexp, rtol=2e-5, atol=2e-5 * np.abs(fexp).max()), (t, force, fexp)
        forces[t] = force
    # the backend's default is timestep 0 (same table, same kernel: equal up to the order of the device's atomic sums), and t = 7 differs
    assert np.allclose(forces[None], forces[0], rtol=1e-6, atol=1e-6 * np.abs(forces[0]).max())
    assert not np.allclose(forces[0], forces[7], rtol=1e-3, atol=0)
    with pytest.raises(Exception, match="runs inside the stepper"):
        bc(f_0, f_1, bc_mask, missing_mask)


@pytest.mark.parametrize("wall", ["hybrid", "halfway"])
def test_momentum_transfer_on_a_static_wall_next_to_a_time_dependent_one(wall):
    """A ramped lid (time-dependent) and a mesh sphere with a static rotation profile in one stepper.  After a run from first_timestep != 0
    that is longer than the ring (timestep 0 never staged, the run's first tables evicted), MomentumTransfer on the sphere reads the
    stepper's single table, with or without timestep=: against the oracle."""
    shape, center, radius = (18, 16, 14), (8.3, 7.6, 6.9), 3.7
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    grid = grid_factory(shape)
    verts = icosphere(center, radius, 1)
    rot, ctr = np.array([0.003, 0.0, -0.004]), np.asarray(center).reshape(3, 1)

    def spin(cells):
        return np.cross(rot.reshape(1, 3), (cells.astype(np.float64) - ctr).T).T

    lid_profile = ramp_lid(shape[0], 3, ramp=1000)
    box_ne = grid.bounding_box_indices(remove_edges=True)
    b_lid = HalfwayBounceBackBC(profile=lid_profile, indices=box_ne["top"])
    method = MeshVoxelizationMethod("RAY")
    if wall == "hybrid":
        b_s = HybridBC("bounceback_regularized", profile=spin, mesh_vertices=verts, voxelization_method=method)
    else:
        b_s = HalfwayBounceBackBC(profile=spin, mesh_vertices=verts, voxelization_method=method)
    assert b_lid.is_time_dependent and not b_s.is_time_dependent
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[b_lid, b_s])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    o_bm, o_mm = orc.build_masks(shape, lat, [orc.BC(orc.KIND_HALFWAY_BB, b_lid.id, box_ne["top"])])
    o_bm, o_mm = mb.mesh_mask_ray(shape, lat, b_s.id, verts, o_bm, o_mm, None)[:2]
    assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
    uw = wall_field(lambda c, t: spin(c), shape, 0)
    o_s = mb.HybridBC(KINDS["bounceback_regularized"], b_s.id, None, u_wall=uw) if wall == "hybrid" else mb.HalfwayProfileBC(b_s.id, None, uw)
    slots = stepper._native_stepper().profile_slots()
    n, t0 = 2 * slots + 7, 5
    f_np = orc.perturbed_init(shape, lat, seed=101, amp_rho=0.01, amp_u=0.02)
    f_0.assign(f_np)
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.4, n, first_timestep=t0)
    out = f_0.numpy()
    exp = oracle_run(f_np, o_bm, o_mm, lambda t: [mb.HalfwayProfileBC(b_lid.id, None, wall_field(lid_profile, shape, t)), o_s], 1.4, lat, t0, n)
    fluid = np.broadcast_to(o_bm != BC_SOLID, out.shape)
    assert np.isfinite(out[fluid]).all() and np.array_equal(out[fluid], exp[fluid])
    with np.errstate(all="ignore"):
        fexp = mb.momentum_transfer(np.where(fluid, out, 0).astype(out.dtype), o_s, o_bm, o_mm, lat)
    assert np.abs(fexp).max() > 0
    for kw in ({}, {"timestep": 3}):
        force = MomentumTransfer(b_s)(f_0, f_1, bc_mask, missing_mask, **kw)
        assert force.shape == (3,) and np.allclose(force, fexp, rtol=2e-5, atol=2e-5 * np.abs(fexp).max()), (kw, force, fexp)


def test_errors_name_the_timestep():
    shape = (12, 10)
    good = ramp_lid(shape[0], 2)

    def bad(cells, t):
        v = good(cells, t)
        return v if t < 4 else v[:, :-1]

    lat, stepper, bc_lid, (f_0, f_1, bc_mask, missing_mask), _ = cavity("D2Q9", shape, bad)  # (t = 0 is fine: prepare_fields passes)
    with pytest.raises(ValueError, match="t=4"):
        stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, 6)
    with pytest.raises(Exception, match="t=5"):
        stepper(f_0, f_1, bc_mask, missing_mask, 1.0, 5)
    # the C ABI: a step whose timestep was never staged fails and leaves the destination untouched
    f_0.assign(orc.perturbed_init(shape, lat, seed=97))
    stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, 2)  # (stages timesteps 0 and 1)
    before = f_1.numpy()
    lib = _lib.load()
    rc = lib.xlbhip_step(stepper._native_stepper()._h, f_0.handle, f_1.handle, bc_mask.handle, missing_mask.handle, 1.0, 12345)
    assert rc != 0 and b"12345" in lib.xlbhip_last_error()
    get_context().sync()
    assert np.array_equal(f_1.numpy(), before)
