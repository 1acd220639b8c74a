#!/usr/bin/env python3
"""What a FlowStatistics sample costs, against Macroscopic on the same field in the same process.

    python tools/stats_bench.py [--cases 0,1,2] [--calls 20] [--reps 3] [--scale 1.0] [--out result.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/stats_bench.py --cases 0 --reps 1      # the kernels on their own

Cases: D3Q19 FP32FP32 at 512^3, D3Q27 FP32FP32 at 384^3, D3Q19 FP32FP16 at 512^3 (``--scale`` shrinks the edge, for a quick look).  Per
case the candidates — ``sample`` with keep_axes (), (2,) and (0,), ``Macroscopic()(f, rho, u)``, and the 16-byte-per-lane copy kernel
of tools/copy_bw.py as the bandwidth yardstick — are warmed up, then timed in turn (``--calls`` calls ended by one synchronisation),
``--reps`` times over, so that whatever state the device is in is shared by all of them.

Condition: the median time of every ``sample`` <= 1.10 x the median time of ``Macroscopic`` (which reads the same q planes and writes
1 + d more).  Reported without a threshold: bytes/s of the traffic model (q s + 1 bytes read per cell) against 8 TB/s and against
the copy kernel's read + write rate, and what the example drivers do today for a profile: Macroscopic + download of u + NumPy mean.
Prints one JSON line per case and a summary table."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.grid import grid_factory
from xlb_amd.operator.macroscopic import Macroscopic
from xlb_amd.operator.postprocess import FlowStatistics
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

CASES = [("D3Q19", "FP32FP32", 512), ("D3Q27", "FP32FP32", 384), ("D3Q19", "FP32FP16", 512)]
KEEPS = [(), (2,), (0,)]


def timed(ctx, fn, calls):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / calls * 1e3


def run_case(lattice, policy, n, calls, reps):
    pp = PrecisionPolicy[policy]
    vs = getattr(xlb.velocity_set, lattice)(precision_policy=pp, compute_backend=ComputeBackend.HIP)
    xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=pp)
    ctx = xlb.default_config.get_context()
    shape = (n, n, n)
    grid = grid_factory(shape)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[])
    f, g, bc_mask, missing_mask = stepper.prepare_fields()  # f: equilibrium at rest; g: the copy's destination
    f, g = stepper.run(f, g, bc_mask, missing_mask, 1.0, 2)
    rho = grid.create_field(1, dtype=pp.compute_precision)
    u = grid.create_field(3, dtype=pp.compute_precision)
    macro = Macroscopic()
    stats = {k: FlowStatistics(grid, keep_axes=k) for k in KEEPS}
    cands = {f"sample{k}": (lambda s=s: s.sample(f, bc_mask)) for k, s in stats.items()}
    cands["macroscopic"] = lambda: macro(f, rho, u)
    cands["copy16"] = lambda: g.copy_kernel_from(f, 16)
    for fn in cands.values():  # warm up this shape
        for _ in range(3):
            fn()
    ctx.sync()
    times = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            times[k].append(timed(ctx, fn, calls))
    # what a driver does today for one profile: Macroscopic, download u, mean of one snapshot
    ctx.sync()
    t0 = time.perf_counter()
    macro(f, rho, u)
    profile = u.numpy()[0].mean(axis=(0, 1))
    host_ms = (time.perf_counter() - t0) * 1e3
    r = stats[(2,)].result()
    cells = n**3
    s_bytes = np.dtype(pp.store_precision.np_dtype).itemsize
    model = cells * (vs.q * s_bytes + 1)
    copy_bytes = 2 * f.info()["plane_stride"] * vs.q * s_bytes
    med = {k: float(np.median(v)) for k, v in times.items()}
    copy_rate = copy_bytes / (med["copy16"] * 1e-3)
    res = {"lattice": lattice, "policy": policy, "shape": shape, "calls": calls, "ms": times, "median_ms": med, "model_bytes": model,
           "copy_read_write_GBps": copy_rate / 1e9, "host_profile_ms": host_ms, "samples": r["samples"], "nonfinite_total": r["nonfinite_total"],
           "profile_agrees": bool(np.allclose(r["u"][0], profile, rtol=1e-5, atol=1e-7))}
    for k in KEEPS:
        t = med[f"sample{k}"]
        res[f"sample{k}"] = {"over_macroscopic": t / med["macroscopic"], "model_GBps": model / (t * 1e-3) / 1e9, "of_8TBps": model / (t * 1e-3) / 8e12,
                             "of_copy": model / (t * 1e-3) / copy_rate}
    res["condition_met"] = all(res[f"sample{k}"]["over_macroscopic"] <= 1.10 for k in KEEPS)
    for obj in (f, g, rho, u, bc_mask, missing_mask):
        obj.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="0,1,2")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 1 or args.reps < 1:
        ap.error("--calls and --reps must be positive")
    results = []
    for i in (int(c) for c in args.cases.split(",")):
        lattice, policy, n = CASES[i]
        res = run_case(lattice, policy, max(16, int(n * args.scale)), args.calls, args.reps)
        print(json.dumps(res), flush=True)
        results.append(res)
    print("\n| case | candidate | ms (each repetition) | x Macroscopic | model GB/s | of 8 TB/s | of the copy |")
    print("|---|---|---|---|---|---|---|")
    for res in results:
        case = f"{res['lattice']} {res['policy']} {res['shape'][0]}^3"
        for k in list(res["ms"]):
            extra = res.get(k)
            cols = [f"{extra['over_macroscopic']:.3f}", f"{extra['model_GBps']:.0f}", f"{extra['of_8TBps']:.3f}", f"{extra['of_copy']:.3f}"] if extra else ["", "", "", ""]
            print(f"| {case} | {k} | {', '.join(f'{t:.3f}' for t in res['ms'][k])} | " + " | ".join(cols) + " |")
        print(f"| {case} | Macroscopic + download + NumPy mean | {res['host_profile_ms']:.0f} | | | | |")
    ok = all(r["condition_met"] for r in results)
    print(f"\ncondition (every sample <= 1.10 x Macroscopic): {'met' if ok else 'MISSED'}")
    if args.out:
        with open(args.out, "w") as fh:
            for res in results:
                fh.write(json.dumps(res) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
