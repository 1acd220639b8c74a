#!/usr/bin/env python3
"""Time the Shan-Chen step (MultiphaseStepper.run) in a fresh process: D3Q19 BGK FP32FP32, size^3 periodic, ShanChenDensity.  Prints one
JSON line with ms/step (host clock around work that ends in a device synchronise) and the algorithmic bytes per cell, (3 q) s + 2 s_c:
k_psi reads q populations and writes psi, k_step_multiphase reads them again with psi and writes q.  The fluid-only figure to set it
against is `bench.py --workload periodic --opt fuse2=0` on the same box in the same call, legs alternated (profiles/multiphase.md).

    python tools/multiphase_bench.py [--size 512] [--steps 200] [--warmup 10] [--form density|exponential|cs] [--psi-only]

--psi-only times the first of the step's two launches alone (k_psi into a field of the caller's: q s + s_c bytes per cell); the second is
the difference to the whole step.
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
from xlb_amd.operator.stepper import CarnahanStarling, MultiphaseStepper, ShanChenDensity, ShanChenExponential

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--form", choices=["density", "exponential", "cs"], default="density")
ap.add_argument("--psi-only", action="store_true", help="time k_psi alone instead of the whole step")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
vs = xlb.velocity_set.D3Q19(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
n = args.size
# a weak interaction on a smooth density wave: the timing does not depend on the values, the run only has to stay finite
model, mean = {"density": (ShanChenDensity(-0.1), 1.0), "exponential": (ShanChenExponential(-3.0), 1.0), "cs": (CarnahanStarling(0.0943 * 1.1), 0.13)}[args.form]
stepper = MultiphaseStepper(grid_factory((n, n, n)), pseudopotential=model)
x = np.arange(n, dtype=np.float32)
wave = 1.0 + 0.01 * np.sin(2 * np.pi * x / n)
rho = (mean * wave[:, None, None] * wave[None, :, None] * wave[None, None, :]).astype(np.float32)
f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields(density=rho)
del rho
ctx = get_context()
f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, args.warmup)
ctx.sync()
if args.psi_only:
    native, psi = stepper._multiphase_native(), grid_factory((n, n, n)).create_field(cardinality=1, dtype=policy.compute_precision)
    native.psi(f_0, bc_mask, missing_mask, psi)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        native.psi(f_0, bc_mask, missing_mask, psi)
    ctx.sync()
    bytes_per_cell = vs.q * 4 + 4
else:
    t0 = time.perf_counter()
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, args.steps)
    ctx.sync()
    bytes_per_cell = 3 * vs.q * 4 + 2 * 4
ms = (time.perf_counter() - t0) * 1e3 / args.steps
print(json.dumps({"workload": f"D3Q19 BGK FP32FP32 periodic {n}^3 Shan-Chen ({args.form}){', k_psi alone' if args.psi_only else ''}", "steps": args.steps, "ms_per_step": round(ms, 4),
                  "mlups": round(n**3 / ms / 1e3, 1), "algorithmic_bytes_per_cell": bytes_per_cell, "achieved_gbs": round(bytes_per_cell * n**3 / ms / 1e6, 1),
                  "finite": bool(np.isfinite(f_0.get_plane(0, n // 2)).all())}))
