#!/usr/bin/env python3
"""Flow past a sphere described by Lagrangian markers (immersed boundary) on the HIP backend: fullway walls, a Regularized velocity
inlet, an extrapolation outflow, KBC collision on D3Q27, and an icosphere whose vertices are coupled to the fluid by IBMStepper.
The drag is the reaction to the coupling forces, -sum_k F_x A_k.

    python examples/sphere_ibm_hip.py [--nx 256 --ny 96 --nz 96] [--radius 10] [--steps 2000] [--re 100]
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
from xlb_amd.helper.ibm_helper import calculate_voronoi_areas, icosphere
from xlb_amd.operator.boundary_condition import ExtrapolationOutflowBC, FullwayBounceBackBC, RegularizedBC
from xlb_amd.operator.macroscopic import Macroscopic
from xlb_amd.operator.stepper import IBMStepper
from xlb_amd.precision_policy import Precision

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=256)
ap.add_argument("--ny", type=int, default=96)
ap.add_argument("--nz", type=int, default=96)
ap.add_argument("--radius", type=float, default=10.0)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--every", type=int, default=0, help="print the drag every so many steps (0: at the end only)")
ap.add_argument("--re", type=float, default=100.0)
ap.add_argument("--u-in", type=float, default=0.04)
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
lattice = xlb.velocity_set.D3Q27(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

shape = (args.nx, args.ny, args.nz)
grid = grid_factory(shape)
box = grid.bounding_box_indices()
box_no_edge = grid.bounding_box_indices(remove_edges=True)
walls = [box["bottom"][i] + box["top"][i] + box["front"][i] + box["back"][i] for i in range(3)]
walls = np.unique(np.array(walls), axis=-1).tolist()

# markers: an icosphere fine enough for about one vertex per cell of surface
subdivisions = 0
while 4.0 * np.pi * args.radius**2 / (10 * 4**subdivisions + 2) > 1.0 and subdivisions < 7:
    subdivisions += 1
unit, faces = icosphere(subdivisions)
centre = np.array([args.nx / 4.0 + 0.3, args.ny / 2.0 + 0.2, args.nz / 2.0 - 0.1])  # off the lattice on purpose
vertices = (unit * args.radius + centre).astype(np.float32)
areas = calculate_voronoi_areas(vertices, faces)
velocities = np.zeros_like(vertices)  # a body at rest

bc_walls = FullwayBounceBackBC(indices=walls)
bc_inlet = RegularizedBC("velocity", prescribed_value=(args.u_in, 0.0, 0.0), indices=box_no_edge["left"])
bc_outlet = ExtrapolationOutflowBC(indices=box_no_edge["right"])
stepper = IBMStepper(grid=grid, boundary_conditions=[bc_walls, bc_inlet, bc_outlet], collision_type="KBC", ibm_max_iterations=4, ibm_tolerance=1e-5)
f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
markers = stepper.markers(vertices, areas, velocities)

visc = args.u_in * (2 * args.radius) / args.re
omega = 1.0 / (3.0 * visc + 0.5)
print(f"grid {shape}, sphere radius {args.radius}, {len(vertices)} markers (sum of areas {areas.sum():.1f}, sphere {4 * np.pi * args.radius**2:.1f}), "
      f"Re {args.re}, omega {omega:.4f}")


def drag():
    forces = stepper.s_lagr_forces.numpy().astype(np.float64)
    return -(forces[:, 0] * areas).sum()


ctx = xlb.default_config.get_context()
t0 = time.perf_counter()
done = 0
while done < args.steps:
    n = min(args.every or args.steps, args.steps - done)
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=done)
    done += n
    if args.every:
        print(f"step {done}: drag {drag():.6e}, sweeps {stepper.ibm_iterations_used}")
ctx.sync()
dt = time.perf_counter() - t0
print(f"{args.steps} steps in {dt:.2f} s: {np.prod(shape) * args.steps / dt / 1e6:.0f} MLUPS, footprint {stepper.ibm_footprint().size} cells of {np.prod(shape)}")

rho = grid.create_field(1, dtype=Precision.FP32)
u = grid.create_field(3, dtype=Precision.FP32)
Macroscopic()(f_0, rho, u)
un, rn = u.numpy(), rho.numpy()
cx, cy, cz = (int(v) for v in centre)
print(f"rho in [{rn.min():.4f}, {rn.max():.4f}], u_x at the centre of the body {un[0, cx, cy, cz]:.5f}, upstream {un[0, cx // 3, cy, cz]:.5f}")
fd = drag()
print(f"drag coefficient {2.0 * fd / (args.u_in**2 * np.pi * args.radius**2):.3f} (channel-confined, rough)")
print(f"drag {fd:.6e}")
assert np.isfinite(un).all() and np.isfinite(fd)
