#!/usr/bin/env python3
"""Time the fused adjoint step (AdjointStepper.backward, one launch per step + the closing launch) and the forward single-step kernel
(IncompressibleNavierStokesStepper.run with fuse2=0) in ONE process, legs alternated: D3Q19 BGK FP32FP32, size^3, periodic or a
lid-driven cavity with halfway walls.  Prints one JSON line: ms/step of both (host clock around work that ends in a device
synchronise), the bytes per cell by the model — 3 q s for the adjoint (f_n, mu in, mu out), 2 q s for the forward step, the masks on
top with walls — the fraction of the 8 TB/s the README uses, and the ratio of the two against the ratio of the byte models (3/2).

    python tools/adjoint_bench.py [--size 512] [--steps 100] [--warmup 5] [--repeats 3] [--walls] [--forward-vec 1]

The backward sweep is timed over `steps` adjoint steps of one forward state (the kernel's work does not depend on the state's values).
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
from xlb_amd.operator.stepper import AdjointStepper, IncompressibleNavierStokesStepper

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--forward-vec", type=int, default=0, help="cells per thread of the forward kernel (0 = its own choice; the adjoint kernel has 1)")
ap.add_argument("--walls", action="store_true", help="a lid-driven cavity with halfway walls instead of the periodic box")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
vs = xlb.velocity_set.D3Q19(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
ctx = get_context()
ctx.set_option("fuse2", 0)  # the forward yardstick is the single-step kernel
ctx.set_option("vec", args.forward_vec)
n = args.size
grid = grid_factory((n, n, n))
bcs = []
if args.walls:
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = [sum((box[f][i] for f in ("bottom", "left", "right", "front", "back")), []) for i in range(3)]
    bcs = [EquilibriumBC(rho=1.0, u=(0.02, 0.0, 0.0), indices=box_ne["top"]), HalfwayBounceBackBC(indices=np.unique(np.array(walls), axis=-1).tolist())]
forward = IncompressibleNavierStokesStepper(grid, boundary_conditions=bcs, backend_config={"lazy_pairs": False})
adjoint = AdjointStepper(forward)
f_0, f_1, bc_mask, missing_mask = forward.prepare_fields()
lam_a, lam_b = adjoint.create_cotangent(), adjoint.create_cotangent()
lam_a.fill(1e-3)
omega = 1.0


def timed(leg, steps):
    ctx.sync()
    t0 = time.perf_counter()
    leg(steps)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def forward_leg(steps):
    global f_0, f_1
    f_0, f_1 = forward.run(f_0, f_1, bc_mask, missing_mask, omega, steps)


def adjoint_leg(steps):
    global lam_a, lam_b
    lam_a, lam_b = adjoint.backward([f_0] * steps, lam_a, lam_b, bc_mask, missing_mask, omega)


forward_leg(args.warmup)
adjoint_leg(args.warmup)
fwd_ms, adj_ms = [], []
for _ in range(args.repeats):
    fwd_ms.append(timed(forward_leg, args.steps))
    adj_ms.append(timed(adjoint_leg, args.steps + 1) * (args.steps + 1) / args.steps)  # steps fused launches + the closing one
d_omega = adjoint.omega_gradient()
s, q, peak = 4, vs.q, 8e12
masks = 5 if args.walls else 0  # bc id + missing word per cell
fwd_bytes, adj_bytes = 2 * q * s + masks, 3 * q * s + masks
fwd, adj = min(fwd_ms), min(adj_ms)
print(json.dumps({"workload": f"D3Q19 BGK FP32FP32 {'cavity (halfway walls)' if args.walls else 'periodic'} {n}^3", "steps": args.steps, "repeats": args.repeats,
                  "forward_vec": args.forward_vec,
                  "forward_ms_per_step": round(fwd, 4), "adjoint_ms_per_step": round(adj, 4), "forward_ms_all": [round(v, 4) for v in fwd_ms],
                  "adjoint_ms_all": [round(v, 4) for v in adj_ms], "forward_bytes_per_cell": fwd_bytes, "adjoint_bytes_per_cell": adj_bytes,
                  "forward_fraction_of_8TBs": round(fwd_bytes * n**3 / (fwd * 1e-3) / peak, 3),
                  "adjoint_fraction_of_8TBs": round(adj_bytes * n**3 / (adj * 1e-3) / peak, 3), "ratio": round(adj / fwd, 3),
                  "byte_model_ratio": round(adj_bytes / fwd_bytes, 3), "finite": bool(np.isfinite(d_omega) and np.isfinite(lam_a.get_plane(0, n // 2)).all())}))
