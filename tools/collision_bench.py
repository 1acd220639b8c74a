#!/usr/bin/env python3
"""Time the single-step kernel with several collisions in ONE process, legs alternated: FP32FP32, size^3, periodic or a lid-driven
cavity with halfway walls, through the stepper's native run (fuse2 = 0, no call pairing: every step is one launch of k_step).  Prints one
JSON line: ms/step per collision (the minimum over the repeats, and all of them), each as a ratio to the first collision listed.

    python tools/collision_bench.py [--lattice D3Q19] [--size 512] [--walls] [--collisions BGK,SmagorinskyLESBGK,RegularizedBGK,RecursiveRegularizedBGK]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import EquilibriumBC, HalfwayBounceBackBC
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

ap = argparse.ArgumentParser()
ap.add_argument("--lattice", default="D3Q19")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--omega", type=float, default=1.7)
ap.add_argument("--walls", action="store_true", help="a lid-driven cavity with halfway walls instead of the periodic box")
ap.add_argument("--collisions", default="BGK,SmagorinskyLESBGK,RegularizedBGK,RecursiveRegularizedBGK")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
vs = getattr(xlb.velocity_set, args.lattice)(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
ctx = get_context()
ctx.set_option("fuse2", 0)
n = args.size
grid = grid_factory((n, n, n))
bcs = []
if args.walls:
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [sum((box[f][i] for f in ("bottom", "left", "right", "front", "back")), []) for i in range(3)]
    bcs = [EquilibriumBC(rho=1.0, u=(0.02, 0.0, 0.0), indices=box_ne["top"]), HalfwayBounceBackBC(indices=np.unique(np.array(walls), axis=-1).tolist())]
names = args.collisions.split(",")
steppers = {c: IncompressibleNavierStokesStepper(grid, boundary_conditions=bcs, collision_type=c, backend_config={"lazy_pairs": False}) for c in names}
# one pair of fields and one pair of masks for all of them (the boundary conditions are the same objects)
f_0, f_1, bc_mask, missing_mask = steppers[names[0]].prepare_fields()


def leg(name, steps):
    global f_0, f_1
    ctx.sync()
    t0 = time.perf_counter()
    f_0, f_1 = steppers[name].run(f_0, f_1, bc_mask, missing_mask, args.omega, steps)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


for c in names:
    leg(c, args.warmup)
ms = {c: [] for c in names}
for _ in range(args.repeats):
    for c in names:
        ms[c].append(leg(c, args.steps))
best = {c: min(v) for c, v in ms.items()}
print(json.dumps({"workload": f"{args.lattice} FP32FP32 {'cavity (halfway walls)' if args.walls else 'periodic'} {n}^3, single-step kernel", "steps": args.steps,
                  "omega": args.omega, "ms_per_step": {c: round(v, 4) for c, v in best.items()}, "ms_all": {c: [round(x, 4) for x in v] for c, v in ms.items()},
                  "ratio_to_" + names[0]: {c: round(best[c] / best[names[0]], 3) for c in names},
                  "finite": bool(np.isfinite(f_0.get_plane(0, n // 2)).all())}))
