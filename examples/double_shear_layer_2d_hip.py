#!/usr/bin/env python3
"""Under-resolved double shear layer (Minion and Brown 1997) on the HIP backend: the case BGK does not survive and the regularised
collisions do.  Fully periodic D2Q9, cell-centre coordinates (i + 1/2) / n:

    ux = u0 tanh(80 (y - 1/4)) for y <= 1/2, u0 tanh(80 (3/4 - y)) above;   uy = 0.05 u0 sin(2 pi (x + 1/4))

at Re = u0 n / nu = 30 000 on n = 64 cells (omega = 1.99898), run for 2 n / u0 steps in FP32FP32.  The script reports the step at
which BGK is lost (non-finite populations or max |u| > 0.5) and the final max |u| of RegularizedBGK and RecursiveRegularizedBGK.

    python examples/double_shear_layer_2d_hip.py [--n 64] [--re 30000] [--u0 0.04]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.grid import grid_factory
from xlb_amd.operator.equilibrium import QuadraticEquilibrium
from xlb_amd.operator.macroscopic import Macroscopic
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--re", type=float, default=30000.0)
ap.add_argument("--u0", type=float, default=0.04)
ap.add_argument("--check-every", type=int, default=100, help="steps between looks at the field")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
lattice = xlb.velocity_set.D2Q9(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

n, u0 = args.n, args.u0
omega = 1.0 / (3.0 * u0 * n / args.re + 0.5)
steps = int(round(2 * n / u0))
grid = grid_factory((n, n))

x, y = np.meshgrid((np.arange(n) + 0.5) / n, (np.arange(n) + 0.5) / n, indexing="ij")
u_init = np.zeros((2, n, n), dtype=np.float32)
u_init[0] = np.where(y <= 0.5, u0 * np.tanh(80.0 * (y - 0.25)), u0 * np.tanh(80.0 * (0.75 - y)))
u_init[1] = 0.05 * u0 * np.sin(2 * np.pi * (x + 0.25))


def max_speed(f):
    """max |u| of the populations, inf when anything is not finite"""
    rho, u = Macroscopic()(f, grid.create_field(1), grid.create_field(2))
    u = u.numpy().astype(np.float64)
    if not (np.isfinite(f.numpy()).all() and np.isfinite(u).all()):
        return float("inf")
    return float(np.sqrt((u * u).sum(axis=0)).max())


def run(collision_type):
    """(step at which the run was lost or None, last max |u|)"""
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type=collision_type)
    f_a, f_b, bc_mask, missing_mask = stepper.prepare_fields()
    rho = grid.create_field(1, fill_value=1.0)
    f_a = QuadraticEquilibrium()(rho, grid.create_field(2).assign(u_init), f_a)
    done, speed = 0, max_speed(f_a)
    while done < steps:
        chunk = min(args.check_every, steps - done)
        f_a, f_b = stepper.run(f_a, f_b, bc_mask, missing_mask, omega, chunk, first_timestep=done)
        done += chunk
        speed = max_speed(f_a)
        if not speed <= 0.5:
            return done, speed
    return None, speed


print(f"double shear layer {n}x{n}, Re = {args.re:g}, u0 = {u0:g}, omega = {omega:.5f}, {steps} steps, FP32FP32")
results = {c: run(c) for c in ("BGK", "RegularizedBGK", "RecursiveRegularizedBGK")}
for name, (lost, speed) in results.items():
    if lost is None:
        print(f"{name}: finite after {steps} steps, max |u| = {speed:.4f}")
    else:
        print(f"{name}: lost by step {lost} (max |u| = {speed:.4g})")
survived = all(results[c][0] is None for c in ("RegularizedBGK", "RecursiveRegularizedBGK"))
print(f"regularised runs survive: {survived}; BGK lost: {results['BGK'][0] is not None}")
