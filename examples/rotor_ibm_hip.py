#!/usr/bin/env python3
"""A turning rotor in a channel, described by Lagrangian markers (immersed boundary) on the HIP backend.

The reference's examples/ibm/wind_turbine_ibm.py reads the turbine from STL files through trimesh and turns the rotor's vertices
with a kernel of its own after every step.  Neither STL files nor trimesh are part of this repository, so the rotor here is
generated: three flat, pitched blades as sheets of markers (area per marker = sheet area / markers) on a cylindrical tower, which
is a second body at rest.  The boundary conditions are those of examples/sphere_ibm_hip.py: fullway walls, a Regularized velocity
inlet, an extrapolation outflow, KBC collision on D3Q27.

The rotor is a body with prescribed motion (RigidMotion about the x axis): the whole run is ONE native call, the markers are moved
on the device, and the force and torque on both bodies are recorded on the device for every step and read once at the end.

    python examples/rotor_ibm_hip.py [--nx 192 --ny 96 --nz 96] [--steps 500] [--tip-speed 0.06] [--pitch 20]

The forcing is under-relaxed (--relaxation 0.5): with 1.0 the forces of moving markers grow without bound within a few steps.  At
the default size and Re 200 the impulsively started flow stayed finite for 750 steps and had blown up by step 950 on an MI355X, so
longer runs want a lower --re or --relaxation (not explored here).
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
from xlb_amd.helper.ibm_helper import IBMBody, RigidMotion
from xlb_amd.operator.boundary_condition import ExtrapolationOutflowBC, FullwayBounceBackBC, RegularizedBC
from xlb_amd.operator.stepper import IBMStepper

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=192)
ap.add_argument("--ny", type=int, default=96)
ap.add_argument("--nz", type=int, default=96)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--every", type=int, default=0, help="print the loads every so many steps (0: at the end only)")
ap.add_argument("--blades", type=int, default=3)
ap.add_argument("--pitch", type=float, default=20.0, help="angle between a blade and the rotor plane, degrees")
ap.add_argument("--tip-speed", type=float, default=0.06, help="speed of the blade tips in lattice units")
ap.add_argument("--u-in", type=float, default=0.04)
ap.add_argument("--relaxation", type=float, default=0.5, help="under-relaxation of the forcing; 1.0 diverges within a few steps for markers that move")
ap.add_argument("--re", type=float, default=200.0, help="Reynolds number on the rotor diameter")
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

# geometry, off the lattice on purpose: the hub on the channel's axis a third of the way down, the tower behind the rotor plane
hub = np.array([args.nx / 3.0 + 0.3, args.ny / 2.0 + 0.2, args.nz / 2.0 - 0.1])
tip = 0.3 * min(args.ny, args.nz)
root, chord = 0.15 * tip, 0.22 * tip
rate = args.tip_speed / tip  # radians per step


def sheet(u_len, v_len):
    """Markers about one cell apart on a u_len x v_len rectangle, as (m, 2) coordinates of the cell centres of the sheet."""
    nu, nv = max(int(round(u_len)), 1), max(int(round(v_len)), 1)
    u, v = np.meshgrid((np.arange(nu) + 0.5) * u_len / nu, (np.arange(nv) + 0.5) * v_len / nv, indexing="ij")
    return np.stack([u.ravel(), v.ravel()], axis=1)


pitch = np.deg2rad(args.pitch)
blade_uv = sheet(tip - root, chord)
blades = []
for b in range(args.blades):
    phi = 2.0 * np.pi * b / args.blades
    radial = np.array([0.0, np.cos(phi), np.sin(phi)])
    tangent = np.array([0.0, -np.sin(phi), np.cos(phi)])
    across = np.cos(pitch) * tangent + np.sin(pitch) * np.array([1.0, 0.0, 0.0])  # the chord direction, pitched out of the rotor plane
    blades.append(hub + (root + blade_uv[:, :1]) * radial + (blade_uv[:, 1:] - chord / 2.0) * across)
rotor = np.concatenate(blades)
rotor_areas = np.full(len(rotor), (tip - root) * chord / len(blade_uv))

tower_radius = max(0.08 * tip, 1.0)
tower_top = hub[2] - root
tower_uv = sheet(2.0 * np.pi * tower_radius, tower_top - 1.5)
angle = tower_uv[:, 0] / tower_radius
tower = np.stack([hub[0] + chord + tower_radius + 1.0 + tower_radius * np.cos(angle), hub[1] + tower_radius * np.sin(angle), 1.5 + tower_uv[:, 1]], axis=1)
tower_areas = np.full(len(tower), 2.0 * np.pi * tower_radius * (tower_top - 1.5) / len(tower))

vertices = np.concatenate([rotor, tower]).astype(np.float32)
areas = np.concatenate([rotor_areas, tower_areas]).astype(np.float32)
velocities = np.zeros_like(vertices)  # (those of the rotor's markers are set on the device)

bc_walls = FullwayBounceBackBC(indices=walls)
bc_inlet = RegularizedBC("velocity", prescribed_value=(args.u_in, 0.0, 0.0), indices=box_no_edge["left"])
bc_outlet = ExtrapolationOutflowBC(indices=box_no_edge["right"])
stepper = IBMStepper(grid=grid, boundary_conditions=[bc_walls, bc_inlet, bc_outlet], collision_type="KBC", ibm_max_iterations=4, ibm_tolerance=1e-5,
                     ibm_relaxation=args.relaxation)
f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
stepper.markers(vertices, areas, velocities)
stepper.set_bodies([IBMBody(markers=slice(0, len(rotor)), motion=RigidMotion(centre=hub, axis=(1.0, 0.0, 0.0), rate=rate)),
                    IBMBody(markers=slice(len(rotor), len(vertices)))])

visc = args.u_in * (2.0 * tip) / args.re
omega = 1.0 / (3.0 * visc + 0.5)
print(f"grid {shape}, rotor: {args.blades} blades of {len(blade_uv)} markers, tip radius {tip:.1f}, pitch {args.pitch:.0f} deg, {rate:.5f} rad/step "
      f"(tip speed ratio {args.tip_speed / args.u_in:.2f}); tower: {len(tower)} markers; Re {args.re}, omega {omega:.4f}")

ctx = xlb.default_config.get_context()
t0 = time.perf_counter()
done = 0
history = []
while done < args.steps:
    n = min(args.every or args.steps, args.steps - done)
    f_0, f_1, loads = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=done, record_loads=True)
    history.append(loads)
    done += n
    if args.every:
        print(f"step {done}: rotor torque {loads[-1, 0, 3]:.6e}, thrust {loads[-1, 0, 0]:.6e}, tower drag {loads[-1, 1, 0]:.6e}, sweeps {stepper.ibm_iterations_used}")
ctx.sync()
dt = time.perf_counter() - t0
history = np.concatenate(history) if history else np.zeros((0, 2, 6))
print(f"{args.steps} steps in {dt:.2f} s: {np.prod(shape) * args.steps / dt / 1e6:.0f} MLUPS, footprint {stepper.ibm_footprint().size} cells of {np.prod(shape)}")

tail = history[-max(args.steps // 10, 1) :]
torque = float(history[-1, 0, 3])  # about the rotor axis (x), on the rotor: negative while the rotor is driven against the fluid
drag = float(history[-1, :, 0].sum())
print(f"mean over the last {len(tail)} steps: torque {tail[:, 0, 3].mean():.6e}, rotor thrust {tail[:, 0, 0].mean():.6e}, tower drag {tail[:, 1, 0].mean():.6e}")
print(f"power {torque * rate:.6e} (torque x rate; positive: the flow drives the rotor)")
print(f"torque {torque:.6e}")
print(f"drag {drag:.6e}")
assert history.shape == (args.steps, 2, 6)
assert np.isfinite(history).all(), f"non-finite loads from step {int(np.argmax(~np.isfinite(history).all(axis=(1, 2))))} on"
assert np.array_equal(history[-1], stepper.body_loads())  # the last row is what body_loads() reads
