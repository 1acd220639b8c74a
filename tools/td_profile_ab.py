"""A / B of a time-dependent wall against the same wall with a static profile (one call, one box).

D3Q19 fp32 lid-driven cavity, halfway walls; the lid is a HalfwayBounceBackBC with a profile, u_x(x) = u0 sin(pi (x + 1/2) / n):
A = profile(cells) (one table for the whole run), B = profile(cells, t) ramped by min(1, (t + 1) / T) (a table per step, evaluated on
the host and staged through the stepper's ring).  Both run the same single-step kernel.  The legs alternate (A B B A ...) after a
warm-up of each; every leg is `stepper.run` of --steps steps timed by the wall clock between two synchronisations (B's host
evaluation overlaps the device, so only a wall clock sees what it costs).  Also timed, chunk by chunk as a run does it: the host
evaluation alone (the profiles into the staging rows) and with the staging call, per step.  One JSON line per size.

    python tools/td_profile_ab.py --sizes 256 512 --steps 200 --rounds 3
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cavity(n, profile):
    from xlb_amd.grid import grid_factory
    from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC
    from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

    grid = grid_factory((n, n, n))
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [sum((box[f][i] for f in ("bottom", "left", "right", "front", "back")), []) for i in range(3)]
    walls = np.unique(np.array(walls), axis=-1).tolist()
    bcs = [HalfwayBounceBackBC(profile=profile, indices=box_ne["top"]), HalfwayBounceBackBC(indices=walls)]
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
    return stepper, list(stepper.prepare_fields())


def lid_profiles(n, u0, ramp):
    """(A, B): profile(cells) and profile(cells, t) — closures, so that A keeps ONE parameter (the arity decides)"""

    def lid(cells):
        u = u0 * np.sin(np.pi * (cells[0].astype(np.float64) + 0.5) / n)
        return np.stack([u, np.zeros_like(u), np.zeros_like(u)])

    def lid_t(cells, t):
        return lid(cells) * min(1.0, (t + 1) / ramp)

    return lid, lid_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()

    import xlb_amd
    from xlb_amd import ComputeBackend, PrecisionPolicy
    from xlb_amd.default_config import get_context
    from xlb_amd.operator.stepper.nse_stepper import chunk_plan

    pp = PrecisionPolicy.FP32FP32
    vs = xlb_amd.velocity_set.D3Q19(precision_policy=pp, compute_backend=ComputeBackend.HIP)
    xlb_amd.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=pp)
    ctx = get_context()
    u0, ramp = 0.05, 10 * args.steps * args.rounds
    for n in args.sizes:
        lid, lid_t = lid_profiles(n, u0, ramp)
        legs = {"A_static": cavity(n, lid), "B_time_dependent": cavity(n, lid_t)}
        assert not legs["A_static"][0]._time_dependent_bcs() and legs["B_time_dependent"][0]._time_dependent_bcs()
        clock = {k: 0 for k in legs}
        ms = {k: [] for k in legs}

        def leg(name, steps, record):
            stepper, f = legs[name]
            ctx.sync()
            t0 = time.perf_counter()
            f[0], f[1] = stepper.run(f[0], f[1], f[2], f[3], 1.0, steps, first_timestep=clock[name])
            ctx.sync()
            clock[name] += steps
            if record:
                ms[name].append((time.perf_counter() - t0) * 1e3 / steps)

        for name in legs:
            leg(name, args.warmup, False)
        order = list(legs)
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                leg(name, args.steps, True)
        # the host's share of B, chunk by chunk as _run_chunked does it (one reused staging buffer): the evaluation alone, then with
        # the staging call (scatter into the pinned image, copy enqueued)
        b = legs["B_time_dependent"][0]
        plan = chunk_plan(args.steps, b._td_slots)
        host = {}
        for with_stage in (False, True):
            ctx.sync()
            t0, t = time.perf_counter(), 0
            for k in plan:
                rows = b._td_rows(t, k)
                if with_stage:
                    b._native.stage_bc_profiles(t, rows)
                t += k
            host[with_stage] = (time.perf_counter() - t0) * 1e3 / args.steps
        ctx.sync()
        host_ms, host_stage_ms = host[False], host[True]
        a_ms, b_ms = statistics.median(ms["A_static"]), statistics.median(ms["B_time_dependent"])
        print(json.dumps({"n": n, "lid_cells": int(b._td_bcs[0]._td_keys.size), "ring_slots": b._td_slots, "steps_per_leg": args.steps,
                          "rounds": args.rounds, "A_ms_per_step": round(a_ms, 4), "B_ms_per_step": round(b_ms, 4),
                          "B_over_A": round(b_ms / a_ms, 4), "host_eval_ms_per_step": round(host_ms, 4), "host_eval_and_stage_ms_per_step": round(host_stage_ms, 4),
                          "A_legs": [round(v, 4) for v in ms["A_static"]], "B_legs": [round(v, 4) for v in ms["B_time_dependent"]]}), flush=True)
        for stepper, f in legs.values():
            for fld in f:
                fld.free()
        del legs


if __name__ == "__main__":
    main()
