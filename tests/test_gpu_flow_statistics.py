"""FlowStatistics on the GPU against the NumPy restatement tests/_stats_ref.py.  Sums: within the derived bound 2 n 2^-53 sum|x| per bin
and channel (two fp64 summations of the same n terms differ by no more, whatever their orders); counts, non-finite counts and the
largest u.u: exactly; run to run, object to object and with or without ghost planes: bit for bit."""

import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC
from xlb_amd.operator.postprocess import FlowStatistics
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper
from xlb_amd.precision_policy import Precision

import _stats_ref as ref
from _util import golden, hip_cavity_3d, init_hip
from test_distributed_gloo import ROOT, free_port

pytestmark = pytest.mark.gpu

SHAPES = {"D3Q19": (37, 22, 70), "D3Q27": (37, 22, 70), "D2Q9": (45, 70)}
KEEPS_3D = [(), (2,), (0,), (0, 2), (1, 2), (0, 1, 2)]
KEEPS_2D = [(), (1,), (0,), (0, 1)]


def flow(lattice, policy, shape, steps=3, seed=3):
    lat = orc.Lattice(lattice)
    f = orc.perturbed_init(shape, lat, policy, seed=seed)
    bm, mm = np.zeros((1,) + tuple(shape), np.uint8), np.zeros((lat.q,) + tuple(shape), bool)
    for _ in range(steps):
        f = orc.step(f, bm, mm, [], 1.3, lat, policy, "BGK")
    return lat, f


def upload(grid, pp, f_np, bm_np=None):
    f = grid.create_field(f_np.shape[0], dtype=pp.store_precision)
    f.assign(f_np)
    bm = None
    if bm_np is not None:
        bm = grid.create_field(1, dtype=Precision.UINT8)
        bm.assign(bm_np)
    return f, bm


def random_mask(shape, seed=11):
    return np.random.default_rng(seed).choice(np.array([0, 0, 0, 1, 7, 255], np.uint8), size=(1,) + tuple(shape))


def check(stats, r, what):
    got = stats.result()
    ref.assert_sums_match(got["sums"], r, what)
    print(f"{what}: max u.u {got['max_u2']!r} / {r['max_u2']!r}, non-finite {got['nonfinite_last']} / {r['nonfinite']}")
    assert got["max_u2"] == r["max_u2"] and got["nonfinite_last"] == r["nonfinite"]
    return got


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64", "FP32FP16"])
@pytest.mark.parametrize("lattice", ["D2Q9", "D3Q19", "D3Q27"])
def test_parity_with_the_restatement(lattice, policy):
    vs, pp = init_hip(lattice, policy)
    shape = SHAPES[lattice]
    lat, f_np = flow(lattice, policy, shape)
    bm_np = random_mask(shape)
    grid = grid_factory(shape)
    f, bm = upload(grid, pp, f_np, bm_np)
    for keep in KEEPS_2D if lat.d == 2 else KEEPS_3D:
        for mask, mask_np, exclude in ((None, None, (255,)), (bm, bm_np, (7, 255))):
            stats = FlowStatistics(grid, keep_axes=keep, exclude_ids=exclude)
            stats.sample(f, mask)
            got = check(stats, ref.restate(f_np, lat, policy, keep, 2, mask_np, exclude), f"{lattice} {policy} keep {keep} mask {mask is not None}")
            assert got["samples"] == stats.samples == 1 and got["rho"].shape == tuple(shape[a] for a in keep)


@pytest.mark.parametrize("keep", KEEPS_3D)
def test_parity_on_a_shape_with_whole_waves(keep):
    vs, pp = init_hip("D3Q19", "FP32FP32")
    shape = (64, 64, 128)
    lat, f_np = flow("D3Q19", "FP32FP32", shape, steps=2)
    grid = grid_factory(shape)
    f, _ = upload(grid, pp, f_np)
    stats = FlowStatistics(grid, keep_axes=keep)
    stats.sample(f)
    check(stats, ref.restate(f_np, lat, "FP32FP32", keep, 2), f"64 x 64 x 128 keep {keep}")


def test_masking_cavity_and_sphere_channel():
    # cavity: lid (1) and walls (2) excluded with 255
    shape = (20, 18, 34)
    grid, bcs, lat, obcs = hip_cavity_3d(shape, HalfwayBounceBackBC)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.2, 6)
    f_np, bm_np = f_0.numpy(), bc_mask.numpy()
    ids = (bcs[0].id, bcs[1].id, 255)
    assert (bm_np != 0).any()
    for keep in ((2,), (0, 1)):
        stats = FlowStatistics(grid, keep_axes=keep, exclude_ids=ids)
        stats.sample(f_0, bc_mask)
        got = check(stats, ref.restate(f_np, lat, "FP32FP32", keep, 2, bm_np, ids), f"cavity keep {keep}")
        summed = tuple(a for a in range(3) if a not in keep)
        assert np.array_equal(got["count"], np.count_nonzero(bm_np[0] == 0, axis=summed))
    # sphere channel: fullway walls (1) and the sphere's cells (4) excluded
    g = golden("d3q19_sphere_channel")
    shape = (28, 14, 14)
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    grid = grid_factory(shape)
    f, bm = upload(grid, pp, g["f"], g["bc_mask"])
    inside = ~np.isin(g["bc_mask"][0], (1, 4, 255))
    for keep in ((0,), ()):
        stats = FlowStatistics(grid, keep_axes=keep, exclude_ids=(1, 4, 255))
        stats.sample(f, bm)
        got = check(stats, ref.restate(g["f"], lat, "FP32FP32", keep, 2, g["bc_mask"], (1, 4, 255)), f"sphere channel keep {keep}")
        assert np.array_equal(got["count"], np.count_nonzero(inside, axis=tuple(a for a in range(3) if a not in keep)))
        # the sums are those of the included cells only
        rho, u = orc.macroscopic(g["f"], lat)
        ux = np.where(inside, u[0], 0).astype(np.float64).sum(axis=tuple(a for a in range(3) if a not in keep))
        assert np.all(np.abs(got["sums"][3] - ux) <= ref.bound(ref.restate(g["f"], lat, "FP32FP32", keep, 2, g["bc_mask"], (1, 4, 255)))[3])


@pytest.mark.parametrize("order", [2, 1])
def test_time_accumulation_reset_and_order(order):
    shape = (20, 18, 34)
    grid, bcs, lat, obcs = hip_cavity_3d(shape, HalfwayBounceBackBC)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_0.assign(orc.perturbed_init(shape, lat, seed=9))
    bm_np = bc_mask.numpy()
    ids = (bcs[1].id, 255)  # the walls
    stats = FlowStatistics(grid, keep_axes=(2,), exclude_ids=ids, order=order)
    total = None
    for i in range(7):
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.4, 1, first_timestep=i)
        stats.sample(f_0, bc_mask)
        total = ref.accumulate(total, ref.restate(f_0.numpy(), lat, "FP32FP32", (2,), order, bm_np, ids))
    got = check(stats, total, f"7 samples, order {order}")
    assert got["samples"] == 7 and got["sums"].shape == (12 if order == 2 else 5, 34)
    n = total["n"].astype(np.float64)
    with np.errstate(all="ignore"):  # (the bottom plane is all wall: no cells, NaN means)
        assert np.array_equal(got["count"], n / 7) and np.array_equal(got["u"][0], got["sums"][3 if order == 2 else 2] / n, equal_nan=True)
    if order == 2:
        rs = stats.reynolds_stress(got)
        assert rs.shape == (6, 34) and np.array_equal(rs[2], got["uu"][2] - got["u"][0] * got["u"][2], equal_nan=True)
    else:
        assert "uu" not in got
    stats.reset()
    empty = stats.result()
    assert empty["samples"] == 0 and not empty["sums"].any() and empty["max_u2"] == 0.0 and empty["nonfinite_total"] == 0
    stats.sample(f_0, bc_mask)
    check(stats, ref.restate(f_0.numpy(), lat, "FP32FP32", (2,), order, bm_np, ids), "after reset")


@pytest.mark.parametrize("keep", [(), (2,), (0,), (0, 2), (1, 2), (0, 1, 2)])
def test_sums_are_bit_reproducible(keep):
    policy, shape = "FP32FP32", (37, 22, 70)
    lat, f_np = flow("D3Q27", policy, shape)
    bm_np = random_mask(shape)
    results = []
    for config in (None, None, {"halo": True}, {"halo": 1}):
        vs, pp = init_hip("D3Q27", policy)
        grid = grid_factory(shape, backend_config=config)
        f, bm = upload(grid, pp, f_np, bm_np)
        assert f.halo == (0 if config is None else (2 if config["halo"] is True else 1))
        stats = FlowStatistics(grid, keep_axes=keep)
        stats.sample(f, bm)
        stats.sample(f, bm)
        first = stats.result()
        second = stats.result()
        assert np.array_equal(first["sums"], second["sums"]) and first["max_u2"] == second["max_u2"]
        assert first["nonfinite_total"] == 0  # ghost planes (zeros: rho = 0) were not sampled
        results.append(first)
    for other in results[1:]:
        assert np.array_equal(results[0]["sums"], other["sums"]) and results[0]["max_u2"] == other["max_u2"]


def test_watchdog_counts_non_finite_cells_and_keeps_them_out_of_the_sums():
    policy, shape = "FP32FP32", (37, 22, 70)
    vs, pp = init_hip("D3Q19", policy)
    lat, f_np = flow("D3Q19", policy, shape)
    bm_np = random_mask(shape)
    cells = [(3, 4, 5), (36, 21, 69), (0, 0, 64)]
    for c in cells:
        bm_np[(0,) + c] = 0
    excluded = tuple(np.argwhere(bm_np[0] == 255)[0])
    bad = f_np.copy()
    bad[5][cells[0]] = np.nan
    bad[0][cells[1]] = np.inf
    bad[7][cells[2]] = -np.inf
    bad[2][excluded] = np.nan
    grid = grid_factory(shape)
    f_bad, bm = upload(grid, pp, bad, bm_np)
    f_ok, _ = upload(grid, pp, f_np)
    for keep in ((), (2,), (0, 1, 2)):
        stats = FlowStatistics(grid, keep_axes=keep)
        stats.sample(f_bad, bm)
        r_bad = ref.restate(bad, lat, policy, keep, 2, bm_np)
        got = check(stats, r_bad, f"watchdog keep {keep}")
        assert got["nonfinite_last"] == got["nonfinite_total"] == 3 and np.isfinite(got["sums"]).all()
        # = the clean field's sums minus those three cells
        holes = bm_np.copy()
        for c in cells:
            holes[(0,) + c] = 255
        ref.assert_sums_match(got["sums"], ref.restate(f_np, lat, policy, keep, 2, holes), "clean field minus the bad cells")
        stats.sample(f_ok, bm)
        again = stats.result()
        assert again["nonfinite_last"] == 0 and again["nonfinite_total"] == 3 and again["max_u2"] == ref.restate(f_np, lat, policy, keep, 2, bm_np)["max_u2"]


def test_samples_are_ordered_with_the_steps_without_host_synchronisation():
    shape = (24, 20, 70)
    runs = []
    for synchronise in (False, True):
        grid, bcs, lat, obcs = hip_cavity_3d(shape, HalfwayBounceBackBC)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        f_0.assign(orc.perturbed_init(shape, lat, seed=4))
        stats = FlowStatistics(grid, keep_axes=(2,), exclude_ids=(bcs[1].id, 255))
        ctx = get_context()
        for i in range(4):
            f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.3, 5, first_timestep=5 * i)
            if synchronise:
                ctx.sync()
            stats.sample(f_0, bc_mask)
            if synchronise:
                ctx.sync()
        runs.append(stats.result())
    assert runs[0]["samples"] == 4 and np.array_equal(runs[0]["sums"], runs[1]["sums"]) and runs[0]["max_u2"] == runs[1]["max_u2"]
    # and a reference-style call that is still deferred is flushed by the sample
    grid, bcs, lat, obcs = hip_cavity_3d(shape, HalfwayBounceBackBC)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_np = orc.perturbed_init(shape, lat, seed=4)
    f_0.assign(f_np)
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, 1.3, 0)
    stats = FlowStatistics(grid, keep_axes=(2,), exclude_ids=(bcs[1].id, 255))
    stats.sample(f_1, bc_mask)
    check(stats, ref.restate(orc.run(f_np, o_bm, o_mm, obcs, 1.3, lat, 1), lat, "FP32FP32", (2,), 2, o_bm, (bcs[1].id, 255)), "deferred step")


def test_failures_name_the_problem():
    vs, pp = init_hip("D3Q19")
    grid, other = grid_factory((12, 10, 16)), grid_factory((12, 10, 18))
    f = grid.create_field(19, dtype=Precision.FP32)
    stats = FlowStatistics(grid, keep_axes=(2,))
    with pytest.raises(Exception, match="not a D3Q19 population field"):
        stats.sample(grid.create_field(27, dtype=Precision.FP32))
    with pytest.raises(Exception, match="made for"):
        stats.sample(other.create_field(19, dtype=Precision.FP32))
    with pytest.raises(Exception, match="another grid"):
        stats.sample(f, other.create_field(1, dtype=Precision.UINT8))
    with pytest.raises(Exception, match="population field"):
        stats.sample(grid.create_field(19, dtype=Precision.UINT8))
    with pytest.raises(Exception, match="uint8"):
        stats.sample(f, grid.create_field(1, dtype=Precision.FP32))
    with pytest.raises(ValueError, match="twice"):
        FlowStatistics(grid, keep_axes=(1, 1))
    with pytest.raises(ValueError, match="out of range"):
        FlowStatistics(grid, keep_axes=(-1,))
    assert stats.samples == 0
    # the C ABI checks on its own
    from xlb_amd import _lib

    stats.sample(f)
    f_other = other.create_field(19, dtype=Precision.FP32)  # (held in a name: the handle of a temporary would outlive its field)
    rc = _lib.load().xlbhip_stats_sample(stats._native._h, f_other.handle, None)
    assert rc != 0 and b"made for 12 x 10 x 16" in _lib.load().xlbhip_last_error()


def test_two_ranks_sharing_one_gpu():
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", XLB_HIP_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "_gpu_stats_rank_worker.py")]
    out = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "GPU_STATS_RANKS_OK" in out.stdout


def test_channel_statistics_example_runs(tmp_path):
    script = os.path.join(ROOT, "examples", "channel_statistics_hip.py")
    res = subprocess.run([sys.executable, script, "--h", "16", "--steps", "300", "--every", "10", "--spin-up", "100"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "20 samples" in res.stdout and "peak of <u'u'>" in res.stdout and "MLUPS" in res.stdout
