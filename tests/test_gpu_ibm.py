"""IBMStepper on the HIP backend against the NumPy restatement of the reference's coupling (tests/_ibm_ref.py, which follows
xlb/operator/stepper/ibm_stepper.py:156-178 and :264-476 on top of the oracle's fluid step).

Tolerance: rho, u and the Lagrangian forces within 1e-6 absolute — the project's graded tolerance for rho / u; the forces are velocity
differences in the same units.  The fp32 and the fp64 restatement differ by up to 6.3e-7 (rho) on these inputs, so any summation
order and the fixed-point accumulation (relative quantum 2^-40 per cell) stay inside; the GPU is compared with the restatement in its OWN compute dtype.

Status: written and rehearsed without a GPU; not yet run on one.  The same kernel sources run thread by thread on the host
(tests/test_ibm_kernels_on_cpu.py) sit at |d rho| <= 6.0e-7, |d u| <= 9.5e-8, |d F| <= 1.2e-7 in fp32 after 10 steps on these inputs."""

import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import ExtrapolationOutflowBC, FullwayBounceBackBC, RegularizedBC
from xlb_amd.operator.stepper import IBMStepper, IncompressibleNavierStokesStepper

import _ibm_ref as ref
from _util import init_hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE = (24, 24, 24)
N_MARKERS = 400
RADIUS = 5.3
CENTRE = (11.3, 12.6, 11.85)
U_BODY = (0.02, 0.01, -0.005)
OMEGA = 1.2
TOL = 1e-6


def body(n=N_MARKERS, centre=CENTRE):
    pos = ref.fibonacci_sphere(n, RADIUS, centre)
    areas = np.full(n, 4 * np.pi * RADIUS**2 / n, dtype=np.float32)
    vel = np.tile(np.array(U_BODY, dtype=np.float32), (n, 1))
    return pos, areas, vel


def periodic_case(lattice, policy, collision, seed=7, **ibm):
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    grid = grid_factory(SHAPE)
    stepper = IBMStepper(grid=grid, boundary_conditions=[], collision_type=collision, **ibm)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_np = orc.perturbed_init(SHAPE, lat, policy, seed=seed)
    f_0.assign(f_np)
    return stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask


def compare(tag, out, forces, exp, lat, policy):
    """rho, u of the field and the forces against the restatement; prints every figure before asserting."""
    T = orc.compute_dtype(policy)
    rho, u = orc.macroscopic(out.astype(T), lat)
    rho_e, u_e = orc.macroscopic(exp["f"].astype(T), lat)
    d_rho = float(np.abs(rho.astype(np.float64) - rho_e).max())
    d_u = float(np.abs(u.astype(np.float64) - u_e).max())
    d_f = float(np.abs(forces.astype(np.float64) - exp["forces"]).max())
    print(f"{tag}: max |d rho| {d_rho:.3e}  max |d u| {d_u:.3e}  max |d F| {d_f:.3e}  (max |F| {np.abs(exp['forces']).max():.3e})")
    assert np.isfinite(out).all()
    assert d_rho <= TOL and d_u <= TOL and d_f <= TOL, (tag, d_rho, d_u, d_f)


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64", "FP64FP32"])
@pytest.mark.parametrize("lattice,collision", [("D3Q19", "BGK"), ("D3Q27", "KBC")])
@pytest.mark.parametrize("steps", [1, 10])
def test_parity_with_the_restatement(lattice, collision, policy, steps):
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = periodic_case(lattice, policy, collision, ibm_max_iterations=4, ibm_relaxation=0.5)
    pos, areas, vel = body()
    o_bm = np.zeros((1,) + SHAPE, np.uint8)
    o_mm = np.zeros((lat.q,) + SHAPE, bool)
    exp = {"f": f_np}
    for i in range(steps):
        f_0, f_1, forces = stepper(f_0, f_1, pos, areas, vel, bc_mask, missing_mask, OMEGA, i)
        f_0, f_1 = f_1, f_0
        exp = ref.step(exp["f"], pos, areas, vel, o_bm, o_mm, [], OMEGA, lat, policy, collision, max_iterations=4, tolerance=1e-5, relaxation=0.5)
    assert exp["sweeps"] == 4 and stepper.ibm_iterations_used == 4
    assert np.abs(exp["G"]).max() > 1e-3  # (the coupling is not a no-op on these inputs)
    compare(f"{lattice} {collision} {policy} {steps} step(s)", f_0.numpy(), forces.numpy(), exp, lat, policy)


def test_cells_outside_the_footprint_are_those_of_the_plain_step():
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = periodic_case("D3Q19", "FP32FP32", "BGK", ibm_relaxation=0.5)
    pos, areas, vel = body()
    stepper(f_0, f_1, pos, areas, vel, bc_mask, missing_mask, OMEGA, 0)
    out = f_1.numpy()
    plain = IncompressibleNavierStokesStepper(grid=stepper.grid, boundary_conditions=[], backend_config={"lazy_pairs": False})
    g_0, g_1, g_bc, g_mm = plain.prepare_fields()
    g_0.assign(f_np)
    plain(g_0, g_1, g_bc, g_mm, OMEGA, 0)
    base = g_1.numpy()
    W = ref.couple(base, pos, areas, vel, lat, "FP32FP32", relaxation=0.5)["W"]
    cells = np.sort(stepper.ibm_footprint())
    assert np.array_equal(cells, np.flatnonzero(W.ravel() > 0))  # the footprint is the set of cells with a positive weight sum
    assert 0 < cells.size < 0.2 * W.size
    outside = W == 0
    assert np.array_equal(out[:, outside], base[:, outside])
    assert not np.array_equal(out[:, ~outside], base[:, ~outside])


def test_bitwise_reproducible_and_independent_of_the_marker_order():
    """acc and W are accumulated as 64-bit fixed-point integers: the sums are exact, so neither the arrival order of the atomics nor
    the order of the markers in the arrays can change a bit."""
    pos, areas, vel = body()
    vel = vel * np.linspace(0.5, 1.5, len(pos), dtype=np.float32)[:, None]
    perm = np.random.default_rng(5).permutation(len(pos))
    results = []
    for order in (None, None, perm):
        stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = periodic_case("D3Q27", "FP32FP32", "KBC", ibm_relaxation=0.5)
        p, a, v = (pos, areas, vel) if order is None else (pos[order], areas[order], vel[order])
        for i in range(3):
            f_0, f_1, forces = stepper(f_0, f_1, p, a, v, bc_mask, missing_mask, OMEGA, i)
            f_0, f_1 = f_1, f_0
        F = forces.numpy()
        if order is not None:
            unpermuted = np.empty_like(F)
            unpermuted[order] = F
            F = unpermuted
        results.append((f_0.numpy(), F))
    for field, F in results[1:]:
        assert np.array_equal(field, results[0][0]) and np.array_equal(F, results[0][1])


@pytest.mark.parametrize("tolerance,max_iterations,expected", [(1e-5, 4, 4), (1.0, 4, 2), (0.0, 6, 6)])
def test_early_exit_is_taken_on_the_device(tolerance, max_iterations, expected):
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = periodic_case("D3Q19", "FP32FP32", "BGK", ibm_max_iterations=max_iterations,
                                                                          ibm_tolerance=tolerance, ibm_relaxation=0.5)
    pos, areas, vel = body()
    _, _, forces = stepper(f_0, f_1, pos, areas, vel, bc_mask, missing_mask, OMEGA, 0)
    o_bm, o_mm = np.zeros((1,) + SHAPE, np.uint8), np.zeros((lat.q,) + SHAPE, bool)
    exp = ref.step(f_np, pos, areas, vel, o_bm, o_mm, [], OMEGA, lat, "FP32FP32", "BGK", max_iterations=max_iterations, tolerance=tolerance, relaxation=0.5)
    assert exp["sweeps"] == expected
    assert stepper.ibm_iterations_used == expected
    compare(f"tolerance {tolerance}, {max_iterations} sweeps", f_1.numpy(), forces.numpy(), exp, lat, "FP32FP32")


CHANNEL = (32, 24, 24)


def channel(policy="FP32FP32", lattice="D3Q19", collision="BGK"):
    """Regularized velocity inlet, extrapolation outflow, fullway walls; the body sits so that its lowest markers are within two cells
    of the wall z = 0 (their support is clipped by the box face and overlaps the wall cells)."""
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    grid = grid_factory(CHANNEL)
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [sum((box[f][i] for f in ("bottom", "top", "front", "back")), []) for i in range(3)]
    walls = np.unique(np.array(walls), axis=-1).tolist()
    u_in = (0.03, 0.0, 0.0)
    b_w = FullwayBounceBackBC(indices=walls)
    b_in = RegularizedBC("velocity", prescribed_value=u_in, indices=box_ne["left"])
    b_out = ExtrapolationOutflowBC(indices=box_ne["right"])
    obcs = [orc.BC(orc.KIND_FULLWAY_BB, b_w.id, walls), orc.BC(orc.KIND_REGULARIZED_VELOCITY, b_in.id, box_ne["left"], prescribed=u_in),
            orc.BC(orc.KIND_EXTRAPOLATION_OUTFLOW, b_out.id, box_ne["right"])]
    stepper = IBMStepper(grid=grid, boundary_conditions=[b_w, b_in, b_out], collision_type=collision, ibm_relaxation=0.5)
    pos, areas, vel = body(centre=(12.4, 11.7, 6.6))
    vel[:] = 0.0  # a body at rest in the stream
    assert pos[:, 2].min() < 2.0
    return stepper, lat, obcs, pos, areas, vel


def test_channel_with_walls_vs_restatement_and_native_run():
    stepper, lat, obcs, pos, areas, vel = channel()
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    o_bm, o_mm = orc.build_masks(CHANNEL, lat, obcs)
    assert np.array_equal(bc_mask.numpy(), o_bm)
    f_np = orc.perturbed_init(CHANNEL, lat, "FP32FP32", seed=11)
    f_0.assign(f_np)
    steps = 6
    exp = {"f": f_np}
    markers = stepper.markers(pos, areas, vel)
    for i in range(steps):
        f_0, f_1, forces = stepper(f_0, f_1, markers, None, None, bc_mask, missing_mask, OMEGA, i)
        f_0, f_1 = f_1, f_0
        exp = ref.step(exp["f"], pos, areas, vel, o_bm, o_mm, obcs, OMEGA, lat, "FP32FP32", "BGK", max_iterations=4, tolerance=1e-5, relaxation=0.5)
    called = f_0.numpy()
    called_forces = forces.numpy()
    compare(f"channel, {steps} calls", called, called_forces, exp, lat, "FP32FP32")
    # the native loop with fixed markers
    f_0.assign(f_np)
    cur, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, steps)
    assert np.array_equal(cur.numpy(), called)
    assert np.array_equal(stepper.s_lagr_forces.numpy(), called_forces)


def test_unsupported_configurations_say_which():
    init_hip("D2Q9")
    with pytest.raises(NotImplementedError, match="2-D"):
        IBMStepper(grid=grid_factory((16, 16)))
    init_hip("D3Q19", "FP32FP16")
    with pytest.raises(NotImplementedError, match="fp16"):
        IBMStepper(grid=grid_factory((8, 8, 8)))
    init_hip("D3Q19")
    with pytest.raises(NotImplementedError, match="slab"):
        IBMStepper(grid=grid_factory((8, 8, 8), backend_config={"halo": 1}))


def test_zero_markers_is_the_plain_step():
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = periodic_case("D3Q19", "FP32FP32", "BGK")
    none = np.zeros((0, 3), np.float32)
    _, _, forces = stepper(f_0, f_1, none, np.zeros(0, np.float32), none, bc_mask, missing_mask, OMEGA, 0)
    with np.errstate(all="ignore"):
        exp = orc.step(f_np, np.zeros((1,) + SHAPE, np.uint8), np.zeros((lat.q,) + SHAPE, bool), [], OMEGA, lat, "FP32FP32", "BGK")
    assert np.array_equal(f_1.numpy(), exp)
    assert forces.numpy().shape == (0, 3) and stepper.ibm_iterations_used == 0


def test_marker_updates_in_place():
    """Velocities replaced on the device, positions kept: the same as passing all three arrays again."""
    pos, areas, vel = body()
    outs = []
    for in_place in (False, True):
        stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = periodic_case("D3Q19", "FP32FP32", "BGK", ibm_relaxation=0.5)
        markers = stepper.markers(pos, areas, vel)
        stepper(f_0, f_1, markers, None, None, bc_mask, missing_mask, OMEGA, 0)
        if in_place:
            markers.update(velocities=2 * vel)
            stepper(f_1, f_0, markers, None, None, bc_mask, missing_mask, OMEGA, 1)
        else:
            stepper(f_1, f_0, pos, areas, 2 * vel, bc_mask, missing_mask, OMEGA, 1)
        outs.append((f_0.numpy(), stepper.s_lagr_forces.numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_sphere_example_runs(tmp_path):
    script = os.path.join(ROOT, "examples", "sphere_ibm_hip.py")
    res = subprocess.run([sys.executable, script, "--nx", "96", "--ny", "48", "--nz", "48", "--radius", "6", "--steps", "50"], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("drag")][-1]
    assert np.isfinite(float(line.split()[-1])), line
