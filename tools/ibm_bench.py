#!/usr/bin/env python3
"""What the immersed-boundary coupling costs: ms/step of IBMStepper against the plain stepper (fuse2 = 0: single steps, which is what an
IBMStepper call runs) on the same grid, alternating the two in one process, on the reference's sphere case (examples/ibm: 525 x 150 x 150,
D3Q27 KBC FP32FP32, radius 25, about one marker per cell of surface).

    python tools/ibm_bench.py [--nx 525 --ny 150 --nz 150 --radius 25] [--steps 100] [--rounds 5] [--out result.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ibm_bench.py --trace-steps 20      # the coupling kernels and their launch sizes

Prints one JSON line: the per-round times, their medians, the footprint and the bytes the coupling moves per step (counted from the
shapes: see coupling_bytes)."""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.grid import grid_factory
from xlb_amd.helper.ibm_helper import calculate_voronoi_areas, icosphere
from xlb_amd.operator.boundary_condition import ExtrapolationOutflowBC, FullwayBounceBackBC, RegularizedBC
from xlb_amd.operator.stepper import IBMStepper, IncompressibleNavierStokesStepper


def coupling_bytes(n_markers, n_slots, q, sweeps, store=4, compute=4):
    """Bytes one call's coupling kernels read + write, from the shapes.  Per slot: moments q S + 4 (cell) + 3 T; correct per sweep
    8 (W) + 24 + 24 (acc read, zeroed) + 3 T (u) + 3 T (G); apply 2 q S + 4 + 3 T.  Per marker-candidate pair (64 per marker): spread per
    sweep after the first 4 (map) + 24 (three 8-byte atomics); interp 4 + 3 T.  Per marker: positions / areas / velocities 28, d and F."""
    T, S = compute, store
    per_slot = (q * S + 4 + 3 * T) + sweeps * (8 + 48 + 6 * T) + (2 * q * S + 4 + 3 * T)
    per_pair = (sweeps - 1) * 28 + (4 + 3 * T)
    per_marker = 28 * 2 + sweeps * 9 * T + 6 * T
    return n_slots * per_slot + 64 * n_markers * per_pair + n_markers * per_marker


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=525)
    ap.add_argument("--ny", type=int, default=150)
    ap.add_argument("--nz", type=int, default=150)
    ap.add_argument("--radius", type=float, default=25.0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--trace-steps", type=int, default=0, help="only run this many IBM steps (for a profiler run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    policy = PrecisionPolicy.FP32FP32
    lattice = xlb.velocity_set.D3Q27(precision_policy=policy, compute_backend=ComputeBackend.HIP)
    xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
    ctx = xlb.default_config.get_context()
    ctx.set_option("fuse2", 0)
    shape = (args.nx, args.ny, args.nz)
    grid = grid_factory(shape)
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [box["bottom"][i] + box["top"][i] + box["front"][i] + box["back"][i] for i in range(3)]
    walls = np.unique(np.array(walls), axis=-1).tolist()
    bcs = [FullwayBounceBackBC(indices=walls), RegularizedBC("velocity", prescribed_value=(0.04, 0.0, 0.0), indices=box_ne["left"]),
           ExtrapolationOutflowBC(indices=box_ne["right"])]
    omega = 1.6

    subdivisions = 0
    while 4.0 * np.pi * args.radius**2 / (10 * 4**subdivisions + 2) > 1.0 and subdivisions < 7:
        subdivisions += 1
    unit, faces = icosphere(subdivisions)
    vertices = (unit * args.radius + np.array([args.nx / 4 + 0.3, args.ny / 2 + 0.2, args.nz / 2 - 0.1])).astype(np.float32)
    areas = calculate_voronoi_areas(vertices, faces)
    velocities = np.zeros_like(vertices)

    ibm = IBMStepper(grid=grid, boundary_conditions=bcs, collision_type="KBC", ibm_max_iterations=args.sweeps, ibm_tolerance=0.0)
    f_0, f_1, bc_mask, missing_mask = ibm.prepare_fields()
    ibm.markers(vertices, areas, velocities)
    if args.trace_steps:
        ibm.run(f_0, f_1, bc_mask, missing_mask, omega, args.trace_steps)
        ctx.sync()
        print(json.dumps({"traced_steps": args.trace_steps, "markers": len(vertices), "footprint_cells": int(ibm.ibm_footprint().size)}))
        return
    plain = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs, collision_type="KBC", backend_config={"lazy_pairs": False})
    g_0, g_1 = grid.create_field(lattice.q), grid.create_field(lattice.q)
    g_0.copy_from(f_0)

    (f_0, f_1), _ = ibm.run_timed(f_0, f_1, bc_mask, missing_mask, omega, args.warmup)
    (g_0, g_1), _ = plain.run_timed(g_0, g_1, bc_mask, missing_mask, omega, args.warmup)
    t_ibm, t_plain = [], []
    for _ in range(args.rounds):  # alternate the two: whatever state the machine is in is shared by both
        (g_0, g_1), ms = plain.run_timed(g_0, g_1, bc_mask, missing_mask, omega, args.steps)
        t_plain.append(ms / args.steps)
        (f_0, f_1), ms = ibm.run_timed(f_0, f_1, bc_mask, missing_mask, omega, args.steps)
        t_ibm.append(ms / args.steps)
    slots = int(ibm.ibm_footprint().size)
    cells = int(np.prod(shape))
    moved = coupling_bytes(len(vertices), slots, lattice.q, args.sweeps)
    med_i, med_p = float(np.median(t_ibm)), float(np.median(t_plain))
    res = {"shape": shape, "markers": len(vertices), "footprint_cells": slots, "footprint_share": slots / cells, "sweeps": args.sweeps,
           "sweeps_used": ibm.ibm_iterations_used, "ms_per_step_plain": t_plain, "ms_per_step_ibm": t_ibm, "median_plain": med_p, "median_ibm": med_i,
           "coupling_ms": med_i - med_p, "coupling_share_of_step": (med_i - med_p) / med_i, "coupling_bytes_per_step": moved,
           "fluid_step_bytes": 2 * lattice.q * 4 * cells, "finite": bool(np.isfinite(f_0.numpy()).all())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
