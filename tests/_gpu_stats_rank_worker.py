"""Worker of tests/test_gpu_flow_statistics.py::test_two_ranks_sharing_one_gpu: FlowStatistics on WORLD_SIZE ranks that share device 0
(host-staged transport), uneven slabs with ghost planes.  With x summed over, result() holds the sums of all ranks on every rank; with
x kept, the ranks' rows concatenated are the single-domain rows.  Both against the single-domain restatement, at its bound."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import xlb_numpy as orc  # noqa: E402
from xlb_amd import distribute as xdist  # noqa: E402
from xlb_amd.grid import grid_factory  # noqa: E402
from xlb_amd.operator.postprocess import FlowStatistics  # noqa: E402
from xlb_amd.precision_policy import Precision  # noqa: E402


def main():
    rank, world = xdist.init_process_group(transport="host")
    import _stats_ref as ref
    from _util import init_hip

    policy, shape = "FP32FP32", (10 * world + 1, 12, 70)
    vs, pp = init_hip("D3Q19", policy)
    lat = orc.Lattice("D3Q19")
    f_np = orc.perturbed_init(shape, lat, policy, seed=21)
    bm0, mm0 = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    f_np = orc.step(f_np, bm0, mm0, [], 1.3, lat, policy, "BGK")
    bm_np = np.random.default_rng(5).choice(np.array([0, 0, 0, 3, 255], np.uint8), size=(1,) + shape)
    grid = grid_factory(shape)
    assert grid.n_ranks == world and grid.halo == 2
    x0, nxl = grid.x_offset, grid.local_shape[0]
    f = grid.create_field(lat.q, dtype=pp.store_precision)
    f.assign(f_np[:, x0 : x0 + nxl])
    bm = grid.create_field(1, dtype=Precision.UINT8)
    bm.assign(bm_np[:, x0 : x0 + nxl])
    ok = True
    for keep in ((2,), (), (1, 2), (0,), (0, 2)):
        stats = FlowStatistics(grid, keep_axes=keep, exclude_ids=(3, 255))
        stats.sample(f, bm)
        stats.sample(f, bm)
        got = stats.result()
        one = ref.restate(f_np, lat, policy, keep, 2, bm_np, (3, 255))
        r = ref.accumulate(ref.accumulate(None, one), one)
        sums = got["sums"]
        if 0 in keep:  # this rank's rows
            good = sums.shape[1] == nxl
            sums = np.concatenate(xdist.all_gather(sums), axis=1)
        else:
            good = all(np.array_equal(sums, other) for other in xdist.all_gather(sums))  # the same bits on every rank
        try:
            ref.assert_sums_match(sums, r, f"rank {rank} keep {keep}")
        except AssertionError as e:
            print(f"rank {rank}: {e}", flush=True)
            good = False
        good = good and got["max_u2"] == r["max_u2"] and got["nonfinite_total"] == 0 and got["samples"] == 2
        if not good:
            print(f"rank {rank}: mismatch with keep {keep}", flush=True)
        ok &= bool(good)
    tot = xdist.all_reduce_sum(0.0 if ok else 1.0)
    if rank == 0:
        print("GPU_STATS_RANKS_OK" if tot == 0 else "GPU_STATS_RANKS_MISMATCH")
    sys.exit(0 if tot == 0 else 1)


if __name__ == "__main__":
    main()
