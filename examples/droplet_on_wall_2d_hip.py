#!/usr/bin/env python3
"""A sessile droplet between two halfway walls on the HIP backend: MultiphaseStepper with the exponential Shan-Chen pseudopotential.
The wall density sets the wetting: a wall density near the liquid's spreads the droplet, one near the vapour's lets it bead up.

    python examples/droplet_on_wall_2d_hip.py [--nx 96] [--ny 40] [--steps 4000] [--wall-density 0.8 1.2 1.8]

Lattice units, D2Q9, FP64FP64, omega = 1, G = -5.5 (liquid about 2.3, vapour about 0.105).  Half a droplet of radius --radius starts on
the bottom wall; x is periodic.  For every wall density the script prints the base width (cells of the wall row above the density
--threshold) and the height (cells of the centre column above it).  A droplet that has left the wall has base width 0.
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
from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC
from xlb_amd.operator.stepper import MultiphaseStepper, ShanChenExponential

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=96)
ap.add_argument("--ny", type=int, default=40)
ap.add_argument("--radius", type=float, default=16.0)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--g", type=float, default=-5.5)
ap.add_argument("--liquid", type=float, default=2.3)
ap.add_argument("--vapour", type=float, default=0.105)
ap.add_argument("--threshold", type=float, default=1.2)
ap.add_argument("--wall-density", type=float, nargs="+", default=[0.8, 1.2, 1.8])
args = ap.parse_args()

policy = PrecisionPolicy.FP64FP64
lattice = xlb.velocity_set.D2Q9(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

nx, ny = args.nx, args.ny
x, y = np.meshgrid(np.arange(nx) + 0.5, np.arange(ny), indexing="ij")
r = np.sqrt((x - 0.5 * nx) ** 2 + y**2)
rho0 = args.vapour + 0.5 * (args.liquid - args.vapour) * (1.0 - np.tanh((r - args.radius) / 2.0))

all_finite = True
for rho_w in args.wall_density:
    grid = grid_factory((nx, ny))
    faces = grid.bounding_box_indices()
    bottom, top = HalfwayBounceBackBC(indices=faces["bottom"]), HalfwayBounceBackBC(indices=faces["top"])
    stepper = MultiphaseStepper(grid, boundary_conditions=[bottom, top], pseudopotential=ShanChenExponential(args.g), wall_density=rho_w)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields(density=rho0)
    # Periodic sides: the masker also flags the directions that leave the box sideways at the walls' two edge columns, which would put a
    # piece of side wall there (and break the conservation of mass).  The walls miss exactly the directions that come out of them.
    missing = missing_mask.numpy()
    missing[:, :, 0] = (lattice.c[1] == 1)[:, None]
    missing[:, :, -1] = (lattice.c[1] == -1)[:, None]
    missing_mask.assign(missing)

    t0 = time.perf_counter()
    f, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, args.steps)
    rho, u = stepper.macroscopic(f, bc_mask, missing_mask)
    rho, u = rho.numpy()[0], u.numpy()
    dt = time.perf_counter() - t0
    finite = bool(np.isfinite(rho).all() and np.isfinite(u).all())
    all_finite = all_finite and finite
    base, height = int((rho[:, 0] > args.threshold).sum()), int((rho[nx // 2, :] > args.threshold).sum())
    print(f"wall density {rho_w:g}: base width {base}, height {height}, rho in [{rho.min():.4f}, {rho.max():.4f}], max |u| = {np.sqrt((u**2).sum(axis=0)).max():.2e}, "
          f"mass {rho.sum():.3f} (start {rho0.sum():.3f}), {args.steps} steps in {dt:.2f} s, fields finite: {finite}")
if not all_finite:
    sys.exit("the fields are not finite")
