#!/usr/bin/env python3
"""2-D Rayleigh-Benard convection on the HIP backend: a hot floor, a cold ceiling, periodic sides — ScalarTransportStepper with
buoyancy (Boussinesq: the force on the fluid is g beta (T - T_ref), the temperature is the transported scalar).

    python examples/rayleigh_benard_2d_hip.py [--ra 1e4] [--pr 0.71] [--nx 128] [--ny 64] [--steps N]

Lattice units: height H = ny (the plates sit half a cell outside the first and the last row), temperature difference 1, free-fall
velocity U = sqrt(g beta H) = --u-ff; then nu = U H sqrt(Pr / Ra), D = nu / Pr.  Prints the Nusselt number from the mean wall-normal
flux at the mid-plane, Nu = <u_y T - D dT/dy> / (D / H): 1 below the critical Rayleigh number 1708, above 1 beyond it.  No
quantitative Nu is claimed here (no reference value was at hand when this was written); the script checks Nu > 1 only when asked to
(--expect-convection) and always that the fields end finite.
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
from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC, ScalarDirichletBC
from xlb_amd.operator.macroscopic import Macroscopic, ScalarMoment
from xlb_amd.operator.stepper import ScalarTransportStepper

ap = argparse.ArgumentParser()
ap.add_argument("--ra", type=float, default=1e4)
ap.add_argument("--pr", type=float, default=0.71)
ap.add_argument("--nx", type=int, default=128)
ap.add_argument("--ny", type=int, default=64)
ap.add_argument("--u-ff", type=float, default=0.05, help="free-fall velocity sqrt(g beta dT H) in lattice units")
ap.add_argument("--steps", type=int, default=0, help="0 = 60 free-fall times H / U")
ap.add_argument("--expect-convection", action="store_true", help="exit non-zero unless Nu > 1")
args = ap.parse_args()

policy = PrecisionPolicy.FP64FP64
lattice = xlb.velocity_set.D2Q9(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

nx, ny = args.nx, args.ny
H = float(ny)
nu = args.u_ff * H * np.sqrt(args.pr / args.ra)
D = nu / args.pr
g_beta = args.u_ff**2 / H
omega = 1.0 / (3.0 * nu + 0.5)
omega_scalar = 1.0 / (3.0 * D + 0.5)  # D2Q5: cs^2 = 1/3
steps = args.steps or int(60 * H / args.u_ff)

grid = grid_factory((nx, ny))
faces = grid.bounding_box_indices()
hot = HalfwayBounceBackBC(indices=faces["bottom"])
cold = HalfwayBounceBackBC(indices=faces["top"])
stepper = ScalarTransportStepper(grid, boundary_conditions=[hot, cold],
                                 scalar_boundary_conditions=[ScalarDirichletBC(1.0, on=hot), ScalarDirichletBC(0.0, on=cold)],
                                 collision_type="BGK", buoyancy=(0.0, g_beta), scalar_reference=0.5)

# the conduction profile plus a small roll-shaped perturbation
x, y = np.meshgrid(np.arange(nx) + 0.5, np.arange(ny) + 0.5, indexing="ij")
T0 = 1.0 - y / H + 1e-2 * np.sin(2 * np.pi * x / nx * max(1, round(nx / (2 * H)))) * np.sin(np.pi * y / H)
f_0, f_1, g_0, g_1, bc_mask, missing_mask = stepper.prepare_fields(scalar=T0)
# Periodic sides: the masker also flags the directions that leave the box sideways at the plates' two edge columns, which would put a
# piece of side wall there.  The plates miss exactly the directions that come out of them.
missing = missing_mask.numpy()
missing[:, :, 0] = (lattice.c[1] == 1)[:, None]
missing[:, :, -1] = (lattice.c[1] == -1)[:, None]
missing_mask.assign(missing)

t0 = time.perf_counter()
f_0, f_1, g_0, g_1 = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, steps)
rho, u = Macroscopic()(f_0, grid.create_field(1, dtype=policy.compute_precision), grid.create_field(2, dtype=policy.compute_precision))
T = ScalarMoment()(g_0, grid.create_field(1, dtype=policy.compute_precision)).numpy()[0]
u = u.numpy()
dt = time.perf_counter() - t0

j = ny // 2  # the two rows around the mid-plane y = H / 2
flux = 0.5 * (u[1, :, j - 1] * T[:, j - 1] + u[1, :, j] * T[:, j]) - D * (T[:, j] - T[:, j - 1])
nusselt = float(flux.mean() / (D / H))
finite = bool(np.isfinite(f_0.numpy()).all() and np.isfinite(g_0.numpy()).all())
print(f"{nx}x{ny} Rayleigh-Benard, Ra={args.ra:g}, Pr={args.pr:g}: nu={nu:.5f} (omega {omega:.4f}), D={D:.5f} (omega_scalar {omega_scalar:.4f}), "
      f"{steps} steps, {nx * ny * steps / dt / 1e6:.0f} MLUPS (launch-bound at this size)")
print(f"Nu = {nusselt:.4f}, max |u| = {np.sqrt((u**2).sum(axis=0)).max():.5f}, T in [{T.min():.4f}, {T.max():.4f}], fields finite: {finite}")
if not finite:
    sys.exit("the fields are not finite")
if args.expect_convection and not nusselt > 1.0:
    sys.exit(f"expected convection (Nu > 1), got Nu = {nusselt:.4f}")
