#!/usr/bin/env python3
"""Time the coupled fluid + scalar step (ScalarTransportStepper.run) in a fresh process: D3Q19 BGK FP32FP32, size^3 periodic, passive
scalar.  Prints one JSON line with ms/step (host clock around work that ends in a device synchronise) and the algorithmic bytes per
cell, 2 (q + 2 d + 1) s.  The fluid-only figure to set it against is `bench.py --workload periodic --opt fuse2=0` on the same box in the
same call, legs alternated (profiles/scalar_transport.md).

    python tools/scalar_bench.py [--size 512] [--steps 200] [--warmup 10] [--buoyancy]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from oracle import xlb_numpy as orc
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.stepper import ScalarTransportStepper

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--buoyancy", action="store_true", help="the forced variant (buoyancy 1e-5 along z) instead of the passive scalar")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
vs = xlb.velocity_set.D3Q19(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
n = args.size
stepper = ScalarTransportStepper(grid_factory((n, n, n)), buoyancy=(0.0, 0.0, 1e-5) if args.buoyancy else None, scalar_reference=1.0)
f_np = orc.perturbed_init((n, n, n), orc.Lattice("D3Q19"), seed=0)
f_0, f_1, g_0, g_1, bc_mask, missing_mask = stepper.prepare_fields(scalar=1.0, initializer=lambda bc_mask, f_0: f_0.assign(f_np))
del f_np
ctx = get_context()
f_0, f_1, g_0, g_1 = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, 1.0, 1.2, args.warmup)
ctx.sync()
t0 = time.perf_counter()
f_0, f_1, g_0, g_1 = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, 1.0, 1.2, args.steps)
ctx.sync()
ms = (time.perf_counter() - t0) * 1e3 / args.steps
bytes_per_cell = 2 * (vs.q + stepper.scalar_q) * 4
print(json.dumps({"workload": f"D3Q19 BGK FP32FP32 periodic {n}^3 + {'buoyant' if args.buoyancy else 'passive'} scalar", "steps": args.steps, "ms_per_step": round(ms, 4),
                  "mlups": round(n**3 / ms / 1e3, 1), "algorithmic_bytes_per_cell": bytes_per_cell, "achieved_gbs": round(bytes_per_cell * n**3 / ms / 1e6, 1),
                  "finite": bool(np.isfinite(g_0.get_plane(0, n // 2)).all())}))
