#!/usr/bin/env python3
"""A droplet of fluid A relaxing inside fluid B on the HIP backend: MulticomponentStepper with the Shan-Chen coupling of two components.

    python examples/droplet_in_fluid_2d_hip.py [--n 64] [--radius 14] [--steps 6000] [--g-ab 2.4] [--omega 1.0 1.0]

Lattice units, D2Q9, FP64FP64, periodic.  Where a component is the majority it starts at --major, where it is the minority at --minor.
The script prints both masses before and after, the radius R (from the area where rho_A is above its mid value), the pressure jump
p_in - p_out of the bulk equation of state and Laplace's product (p_in - p_out) R, which is the surface tension in two dimensions.
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.grid import grid_factory
from xlb_amd.operator.stepper import MulticomponentStepper, ShanChenMixture

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--radius", type=float, default=14.0)
ap.add_argument("--steps", type=int, default=6000)
ap.add_argument("--g-ab", type=float, default=2.4)
ap.add_argument("--major", type=float, default=1.0)
ap.add_argument("--minor", type=float, default=0.04)
ap.add_argument("--omega", type=float, nargs=2, default=[1.0, 1.0])
args = ap.parse_args()

policy = PrecisionPolicy.FP64FP64
lattice = xlb.velocity_set.D2Q9(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

n = args.n
x, y = np.meshgrid(np.arange(n) + 0.5, np.arange(n) + 0.5, indexing="ij")
r = np.sqrt((x - 0.5 * n) ** 2 + (y - 0.5 * n) ** 2)
inside = 0.5 * (1.0 - np.tanh((r - args.radius) / 2.0))
rho_a0 = args.minor + (args.major - args.minor) * inside
rho_b0 = args.minor + (args.major - args.minor) * (1.0 - inside)

mixture = ShanChenMixture(G_AB=args.g_ab)
stepper = MulticomponentStepper(grid_factory((n, n)), interaction=mixture)
fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask = stepper.prepare_fields(density=(rho_a0, rho_b0))

t0 = time.perf_counter()
fa, _, fb, _ = stepper.run(fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, tuple(args.omega), args.steps)
rho_a, rho_b, u = (field.numpy() for field in stepper.macroscopic(fa, fb, bc_mask, missing_mask))
dt = time.perf_counter() - t0
rho_a, rho_b = rho_a[0], rho_b[0]
finite = bool(np.isfinite(rho_a).all() and np.isfinite(rho_b).all() and np.isfinite(u).all())

c = n // 2
radius = np.sqrt(float((rho_a > 0.5 * (rho_a[c, c] + rho_a[0, 0])).sum()) / np.pi)
jump = float(mixture.pressure(rho_a[c, c], rho_b[c, c]) - mixture.pressure(rho_a[0, 0], rho_b[0, 0]))
print(f"droplet of A in B, {n} x {n}, G_AB = {args.g_ab:g}, omega = ({args.omega[0]:g}, {args.omega[1]:g}), {args.steps} steps in {dt:.2f} s")
print(f"mass of A: {rho_a0.sum():.6f} -> {rho_a.sum():.6f}")
print(f"mass of B: {rho_b0.sum():.6f} -> {rho_b.sum():.6f}")
print(f"inside (rho_A, rho_B) = ({rho_a[c, c]:.4f}, {rho_b[c, c]:.4f}), outside ({rho_a[0, 0]:.4f}, {rho_b[0, 0]:.4f}), max |u| = {np.sqrt((u**2).sum(axis=0)).max():.2e}")
print(f"R = {radius:.3f}, p_in - p_out = {jump:.5e}, Laplace product (p_in - p_out) R = {jump * radius:.5f}, fields finite: {finite}")
if not finite:
    sys.exit("the fields are not finite")
