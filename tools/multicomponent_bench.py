#!/usr/bin/env python3
"""Time the two-component Shan-Chen step (MulticomponentStepper.run) in a fresh process: D3Q19 BGK FP32FP32, size^3 periodic.  Prints one
JSON line with ms/step (host clock around work that ends in a device synchronise) and the algorithmic bytes per cell, 2 (3 q) s + 4 s_c:
k_mix_density reads both sets and writes both densities, k_mix_step reads both sets again with both densities and writes both sets.  The
single-component figure to set it against is `tools/multiphase_bench.py` (236 B per cell) on the same box in the same call, legs
alternated (profiles/multicomponent.md).

    python tools/multicomponent_bench.py [--size 512] [--steps 200] [--warmup 10] [--density-only]

--density-only times the first of the step's two launches alone (k_mix_density into fields of the caller's: 2 q s + 2 s_c bytes per
cell); the second is the difference to the whole step.
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
from xlb_amd.operator.stepper import MulticomponentStepper, ShanChenMixture

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--density-only", action="store_true", help="time k_mix_density alone instead of the whole step")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
vs = xlb.velocity_set.D3Q19(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
n = args.size
# a weak interaction on smooth density waves: the timing does not depend on the values, the run only has to stay finite
stepper = MulticomponentStepper(grid_factory((n, n, n)), interaction=ShanChenMixture(G_AB=0.1, G_AA=-0.05, G_BB=0.05))
x = np.arange(n, dtype=np.float32)
wave = 1.0 + 0.01 * np.sin(2 * np.pi * x / n)
rho_a = (0.6 * wave[:, None, None] * wave[None, :, None] * wave[None, None, :]).astype(np.float32)
fields = stepper.prepare_fields(density=(rho_a, (1.0 - rho_a).astype(np.float32)))
fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask = fields
del rho_a
ctx = get_context()
omega = (1.0, 1.4)
fa_0, fa_1, fb_0, fb_1 = stepper.run(fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega, args.warmup)
ctx.sync()
if args.density_only:
    grid = grid_factory((n, n, n))
    native = stepper._multicomponent_native()
    rho = [grid.create_field(cardinality=1, dtype=policy.compute_precision) for _ in range(2)]
    native.densities(fa_0, fb_0, bc_mask, missing_mask, *rho)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        native.densities(fa_0, fb_0, bc_mask, missing_mask, *rho)
    ctx.sync()
    bytes_per_cell = 2 * vs.q * 4 + 2 * 4
else:
    t0 = time.perf_counter()
    fa_0, fa_1, fb_0, fb_1 = stepper.run(fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega, args.steps)
    ctx.sync()
    bytes_per_cell = 2 * 3 * vs.q * 4 + 4 * 4
ms = (time.perf_counter() - t0) * 1e3 / args.steps
finite = bool(np.isfinite(fa_0.get_plane(0, n // 2)).all() and np.isfinite(fb_0.get_plane(0, n // 2)).all())
print(json.dumps({"workload": f"D3Q19 BGK FP32FP32 periodic {n}^3 two-component Shan-Chen{', k_mix_density alone' if args.density_only else ''}", "steps": args.steps,
                  "ms_per_step": round(ms, 4), "mlups": round(n**3 / ms / 1e3, 1), "algorithmic_bytes_per_cell": bytes_per_cell,
                  "achieved_gbs": round(bytes_per_cell * n**3 / ms / 1e6, 1), "finite": finite}))
