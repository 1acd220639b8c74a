#!/usr/bin/env python3
"""Time the porous forward step against the plain single-step kernel (fuse2=0) and the porous adjoint sweep against the plain adjoint
sweep in ONE process, legs alternated (tools/adjoint_bench.py's method): D3Q19 BGK FP32FP32, size^3, periodic or a lid-driven cavity
with halfway walls, alpha seeded in [0, 0.9].  Prints one JSON line: ms/step of the four legs (minimum of `repeats`, all recorded; host
clock around work that ends in a device synchronise), the bytes per cell by the models — forward 2 q s + s_c against 2 q s, adjoint
3 q s + s_c + 16 against 3 q s, the masks on top with walls — and the measured ratios next to the models'.

    python tools/porous_bench.py [--size 512] [--steps 100] [--warmup 5] [--repeats 3] [--walls]

The four steppers share the population fields and the masks (each family starts a fresh id registry, so that its boundary conditions get
the same ids).  The sweeps are timed over `steps` adjoint steps of one forward state."""

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
from xlb_amd.operator.boundary_condition import EquilibriumBC, HalfwayBounceBackBC, boundary_condition_registry
from xlb_amd.operator.stepper import AdjointStepper, IncompressibleNavierStokesStepper, PorousStepper

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--walls", action="store_true", help="a lid-driven cavity with halfway walls instead of the periodic box")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
n = args.size


def family(make):
    """a stepper on a fresh id registry: the boundary conditions of every family get the ids 1, 2"""
    boundary_condition_registry.__init__()
    vs = xlb.velocity_set.D3Q19(precision_policy=policy, compute_backend=ComputeBackend.HIP)
    xlb.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
    grid = grid_factory((n, n, n))
    bcs = []
    if args.walls:
        box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
        walls = [sum((box[f][i] for f in ("bottom", "left", "right", "front", "back")), []) for i in range(3)]
        bcs = [EquilibriumBC(rho=1.0, u=(0.02, 0.0, 0.0), indices=box_ne["top"]), HalfwayBounceBackBC(indices=np.unique(np.array(walls), axis=-1).tolist())]
    return vs, make(grid, bcs)


vs, plain = family(lambda grid, bcs: IncompressibleNavierStokesStepper(grid, boundary_conditions=bcs, backend_config={"lazy_pairs": False}))
_, porous = family(lambda grid, bcs: PorousStepper(grid, boundary_conditions=bcs))
ctx = get_context()
ctx.set_option("fuse2", 0)  # the forward yardstick is the single-step kernel
f_0, f_1, bc_mask, missing_mask = plain.prepare_fields()
alpha = porous.create_solidity()
rng = np.random.default_rng(17)
for x in range(n):  # plane by plane: a whole 512^3 host array is not needed
    alpha.set_plane(0, x, rng.uniform(0.0, 0.9, (n, n)).astype(np.float32))
porous.set_solidity(alpha)
adjoints = {"plain": AdjointStepper(plain), "porous": AdjointStepper(porous)}
lam_a, lam_b = adjoints["plain"].create_cotangent(), adjoints["plain"].create_cotangent()
lam_a.fill(1e-3)
omega = 1.0


def timed(leg, steps):
    ctx.sync()
    t0 = time.perf_counter()
    leg(steps)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def forward_leg(stepper):
    def leg(steps):
        global f_0, f_1
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, steps)

    return leg


def adjoint_leg(name):
    def leg(steps):
        global lam_a, lam_b
        lam_a, lam_b = adjoints[name].backward([f_0] * steps, lam_a, lam_b, bc_mask, missing_mask, omega)

    return leg


legs = {"forward_plain": forward_leg(plain), "forward_porous": forward_leg(porous), "adjoint_plain": adjoint_leg("plain"), "adjoint_porous": adjoint_leg("porous")}
for leg in legs.values():
    leg(args.warmup)
ms = {k: [] for k in legs}
for _ in range(args.repeats):
    for k, leg in legs.items():
        if k.startswith("adjoint"):
            ms[k].append(timed(leg, args.steps + 1) * (args.steps + 1) / args.steps)  # steps fused launches + the closing one
        else:
            ms[k].append(timed(leg, args.steps))
s, sc, q = 4, 4, vs.q
masks = 5 if args.walls else 0  # bc id + missing word per cell
model = {"forward_plain": 2 * q * s + masks, "forward_porous": 2 * q * s + sc + masks, "adjoint_plain": 3 * q * s + masks, "adjoint_porous": 3 * q * s + sc + 16 + masks}
best = {k: min(v) for k, v in ms.items()}
g = adjoints["porous"].solidity_gradient()
finite = bool(np.isfinite(g.get_plane(0, n // 2)).all() and np.isfinite(lam_a.get_plane(0, n // 2)).all() and np.isfinite(f_0.get_plane(0, n // 2)).all())
print(json.dumps({"workload": f"D3Q19 BGK FP32FP32 {'cavity (halfway walls)' if args.walls else 'periodic'} {n}^3", "steps": args.steps, "repeats": args.repeats,
                  "ms_per_step": {k: round(v, 4) for k, v in best.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                  "bytes_per_cell": model,
                  "forward_ratio": round(best["forward_porous"] / best["forward_plain"], 3),
                  "forward_model_ratio": round(model["forward_porous"] / model["forward_plain"], 3),
                  "adjoint_ratio": round(best["adjoint_porous"] / best["adjoint_plain"], 3),
                  "adjoint_model_ratio": round(model["adjoint_porous"] / model["adjoint_plain"], 3),
                  "porous_adjoint_over_porous_forward": round(best["adjoint_porous"] / best["forward_porous"], 3),
                  "plain_adjoint_over_plain_forward": round(best["adjoint_plain"] / best["forward_plain"], 3), "finite": finite}))
