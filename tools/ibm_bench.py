#!/usr/bin/env python3
"""What the immersed-boundary coupling costs: ms/step of IBMStepper against the plain stepper (fuse2 = 0: single steps, which is what an
IBMStepper call runs) on the same grid, alternating the two in one process, on the reference's sphere case (examples/ibm: 525 x 150 x 150,
D3Q27 KBC FP32FP32, radius 25, about one marker per cell of surface).

    python tools/ibm_bench.py [--nx 525 --ny 150 --nz 150 --radius 25] [--steps 100] [--rounds 5] [--out result.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ibm_bench.py --trace-steps 20      # the coupling kernels and their launch sizes

Prints one JSON line: the per-round times, their medians, the footprint and the bytes the coupling moves per step (counted from the
shapes: see coupling_bytes).

    python tools/ibm_bench.py --moving [--steps 100 --rounds 5]     # the same sphere spinning about its own axis
    python tools/ibm_bench.py --moving --counted-only               # no GPU: what move / rebuild / loads add per step, from the shapes

--moving times, interleaved, (a) the loop the host drives — NumPy kinematics, markers.update(vertices, velocities) and one call per
step —, (b) the native run with the sphere declared as a body with a RigidMotion and (c) the native run with the markers at rest, and
reports (a) and (b) in ms/step and (b - c) / b, the share of the step that moving the markers, rebuilding the footprint and summing
the loads take.

    python tools/ibm_bench.py --dynamics [--steps 100 --rounds 5]   # the --moving sphere as a FREE body against the prescribed one
    python tools/ibm_bench.py --dynamics --counted-only             # no GPU: the two launches a free body adds, and their bytes

--dynamics times, interleaved round by round (the bodies are declared before the clock starts), the native run of the sphere as a
body with a RigidMotion (what --moving calls "native") and the native run of the same sphere declared with a RigidDynamics (heavy, spinning at --rate, so that it moves as the
prescribed one does), and reports both medians, the spread of each and their difference: what k_ibm_pose and k_ibm_integrate cost."""

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


def moving_counts(n_markers, n_slots, n_bodies=1, compute=4, cap=None):
    """Launches and bytes one step of a MOVING body adds to the call, from the shapes (csrc/ibm.hip: ibm_move, ibm_build_footprint,
    ibm_body_loads).  move: per marker 12 (X0) + 4 (body id) read, 12 + 12 written.  rebuild: k_ibm_clear 8 per slot in use; three
    memsets over the slot CAPACITY (wbits 4, W 8, acc 24 per slot) and one of 4 bytes; mark / wmax / weights per marker-candidate
    pair 4 + (4 + 4) + (4 + 4 + 8), per slot in use 8 (list, map), per marker 3 x 12 (positions).  loads: per marker 3 T + 4 + 12
    read, per chunk of 256 markers 48 written and read, per body 48 written (twice when a history is recorded).  Poses: 144 bytes
    per body and step cross the host link, one copy per chunk of up to 256 steps."""
    cap = min(64 * n_markers, cap) if cap else 64 * n_markers
    chunks = n_bodies * -(-(n_markers // n_bodies) // 256)
    move = {"launches": 1, "bytes": n_markers * 40}
    rebuild = {"launches": 8, "kernels": 4, "memsets": 4, "bytes": n_slots * 8 + cap * 36 + 4 + 64 * n_markers * 28 + n_slots * 8 + n_markers * 36,
               "of_which_memsets_over_the_capacity": cap * 36}
    loads = {"launches": 2, "bytes": n_markers * (3 * compute + 16) + chunks * 96 + n_bodies * 96}
    return {"move": move, "rebuild": rebuild, "loads": loads, "launches_added": 11, "bytes_added": move["bytes"] + rebuild["bytes"] + loads["bytes"],
            "pose_bytes_over_the_host_link": 144 * n_bodies}


def dynamics_counts(n_bodies=1, recorded=False):
    """Launches and bytes one step of a run with FREE bodies adds on top of moving_counts (csrc/ibm.hip: ibm_live_pose,
    ibm_integrate), per body.  k_ibm_pose: 8 (kind, rotate) + 128 (state) + 256 (parameters) read — or 144 of a staged / rest row —,
    144 written (twice when a history is recorded).  k_ibm_integrate: 8 + 256 + 128 + 48 (loads) read, 104 written (13 doubles of
    state).  No pose crosses the host link."""
    pose = {"launches": 1, "blocks": 1, "threads": 64, "bytes": n_bodies * (8 + 128 + 256 + 144 * (2 if recorded else 1))}
    integrate = {"launches": 1, "blocks": 1, "threads": 64, "bytes": n_bodies * (8 + 256 + 128 + 48 + 104)}
    return {"pose": pose, "integrate": integrate, "launches_added": 2, "bytes_added": pose["bytes"] + integrate["bytes"], "pose_bytes_over_the_host_link": 0}


def bench_dynamics(args, ctx, ibm, make_fields, vertices, velocities, centre, omega):
    from xlb_amd.helper.ibm_helper import IBMBody, RigidDynamics, RigidMotion

    f_0, f_1, bc_mask, missing_mask = make_fields()
    markers = ibm._markers
    clock = [0]

    def timed(fn):
        import time

        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return out, (time.perf_counter() - t0) * 1e3

    def declare(bodies):  # set-up, outside the timed region: uploads, allocations and a stream synchronise that differ between the legs
        markers.update(vertices=vertices, velocities=velocities)
        ibm.set_bodies(bodies)

    def native(f_0, f_1, n):
        out = ibm.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=clock[0])
        clock[0] += n
        return out

    def prescribed():
        return [IBMBody(markers=slice(0, len(vertices)), motion=RigidMotion(centre=centre, axis=(0.0, 0.0, 1.0), rate=args.rate))]

    def free():
        # heavy enough for the loads not to matter within a round: it spins on at --rate as the prescribed sphere does
        volume = 4.0 / 3.0 * np.pi * args.radius**3
        dyn = RigidDynamics(mass=1e3 * volume, inertia=1e3 * 0.4 * volume * args.radius**2, centre=centre, angular_velocity=(0.0, 0.0, args.rate))
        return [IBMBody(markers=slice(0, len(vertices)), dynamics=dyn)]

    times = {"prescribed": [], "dynamics": []}
    for bodies in (prescribed(), free()):
        declare(bodies)
        f_0, f_1 = native(f_0, f_1, args.warmup)
    for r in range(args.rounds):  # interleaved, the order alternating: whatever state the machine is in is shared by the two
        for name in (("prescribed", "dynamics") if r % 2 == 0 else ("dynamics", "prescribed")):
            declare(prescribed() if name == "prescribed" else free())
            (f_0, f_1), ms = timed(lambda: native(f_0, f_1, args.steps))
            times[name].append(ms / args.steps)
    pose = ibm.body_poses()[0]
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float(np.max(v) - np.min(v)) for k, v in times.items()}
    slots = int(ibm.ibm_footprint().size)
    return {"dynamics": True, "markers": len(vertices), "rate": args.rate, "footprint_cells": slots, "ms_per_step": times, "median_prescribed": med["prescribed"],
            "median_dynamics": med["dynamics"], "spread_prescribed": spread["prescribed"], "spread_dynamics": spread["dynamics"],
            "dynamics_minus_prescribed_ms": med["dynamics"] - med["prescribed"], "counted": dynamics_counts(), "final_rate": float(pose[14]),
            "finite": bool(np.isfinite(f_0.numpy()).all())}


def bench_moving(args, ctx, ibm, make_fields, vertices, velocities, centre, omega):
    from xlb_amd.helper.ibm_helper import IBMBody, RigidMotion

    motion = RigidMotion(centre=centre, axis=(0.0, 0.0, 1.0), rate=args.rate)
    f_0, f_1, bc_mask, missing_mask = make_fields()
    markers = ibm._markers
    x0 = vertices.astype(np.float64) - centre
    clock = [0]

    def host_loop(f_0, f_1, n):
        for _ in range(n):
            t = clock[0]
            R, c, w, v = motion.at(t)
            x = x0 @ R.T
            markers.update(vertices=(x + c).astype(np.float32), velocities=(v + np.cross(w, x)).astype(np.float32))
            ibm(f_0, f_1, markers, None, None, bc_mask, missing_mask, omega, t)
            f_0, f_1 = f_1, f_0
            clock[0] += 1
        return f_0, f_1

    def timed(fn):
        import time

        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        return out, (time.perf_counter() - t0) * 1e3

    def native(f_0, f_1, n, bodies):
        markers.update(vertices=vertices, velocities=velocities)
        ibm.set_bodies(bodies)
        out = ibm.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=clock[0])
        clock[0] += n
        return out

    body = [IBMBody(markers=slice(0, len(vertices)), motion=motion)]
    times = {"host_loop": [], "native": [], "at_rest": []}
    f_0, f_1 = host_loop(f_0, f_1, args.warmup)
    f_0, f_1 = native(f_0, f_1, args.warmup, body)
    for _ in range(args.rounds):  # interleaved: whatever state the machine is in is shared by the three
        ibm.set_bodies([])
        (f_0, f_1), ms = timed(lambda: host_loop(f_0, f_1, args.steps))
        times["host_loop"].append(ms / args.steps)
        (f_0, f_1), ms = timed(lambda: native(f_0, f_1, args.steps, body))
        times["native"].append(ms / args.steps)
        (f_0, f_1), ms = timed(lambda: native(f_0, f_1, args.steps, []))
        times["at_rest"].append(ms / args.steps)
    med = {k: float(np.median(v)) for k, v in times.items()}
    slots = int(ibm.ibm_footprint().size)
    return {"moving": True, "markers": len(vertices), "rate": args.rate, "footprint_cells": slots, "ms_per_step": times, "median_host_loop": med["host_loop"],
            "median_native": med["native"], "median_at_rest": med["at_rest"], "native_over_host_loop": med["native"] / med["host_loop"],
            "move_rebuild_loads_share_of_step": (med["native"] - med["at_rest"]) / med["native"], "counted": moving_counts(len(vertices), slots),
            "finite": bool(np.isfinite(f_0.numpy()).all())}


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
    ap.add_argument("--moving", action="store_true", help="the sphere spins about its own axis: host-driven loop against the native run")
    ap.add_argument("--dynamics", action="store_true", help="the --moving sphere as a free body: native run against the prescribed native run")
    ap.add_argument("--rate", type=float, default=0.002, help="--moving: radians per step (surface speed = rate x radius)")
    ap.add_argument("--counted-only", action="store_true", help="--moving: print what is counted from the shapes and stop (no GPU needed)")
    ap.add_argument("--footprint-cells", type=int, default=43316, help="--counted-only: the footprint (profiles/ibm_coupling.md has the bench case's)")
    args = ap.parse_args()

    if args.dynamics and args.counted_only:
        print(json.dumps({"bodies": 1, "counted": dynamics_counts(), "counted_with_a_recorded_history": dynamics_counts(recorded=True)}))
        return
    if args.moving and args.counted_only:
        subdivisions = 0
        while 4.0 * np.pi * args.radius**2 / (10 * 4**subdivisions + 2) > 1.0 and subdivisions < 7:
            subdivisions += 1
        print(json.dumps({"markers": 10 * 4**subdivisions + 2, "footprint_cells": args.footprint_cells,
                          "counted": moving_counts(10 * 4**subdivisions + 2, args.footprint_cells, cap=args.nx * args.ny * args.nz)}))
        return

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
    centre = np.array([args.nx / 4 + 0.3, args.ny / 2 + 0.2, args.nz / 2 - 0.1])
    vertices = (unit * args.radius + centre).astype(np.float32)
    areas = calculate_voronoi_areas(vertices, faces)
    velocities = np.zeros_like(vertices)

    ibm = IBMStepper(grid=grid, boundary_conditions=bcs, collision_type="KBC", ibm_max_iterations=args.sweeps, ibm_tolerance=0.0)
    f_0, f_1, bc_mask, missing_mask = ibm.prepare_fields()
    ibm.markers(vertices, areas, velocities)
    if args.dynamics:
        line = json.dumps(bench_dynamics(args, ctx, ibm, lambda: (f_0, f_1, bc_mask, missing_mask), vertices, velocities, centre, omega))
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    if args.moving:
        line = json.dumps(bench_moving(args, ctx, ibm, lambda: (f_0, f_1, bc_mask, missing_mask), vertices, velocities, centre, omega))
        print(line)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
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
