#!/usr/bin/env python3
"""A heavy sphere released from rest in a closed box of fluid at rest: a FREE immersed-boundary body on the HIP backend.

The sphere is an icosphere of Lagrangian markers declared as a body with ``RigidDynamics.sphere`` (Uhlmann's effective mass and
weight, J. Comput. Phys. 209 (2005) 448): after every step the device sums the force on the body and advances its centre and
velocity from it, and the next step places the markers there.  Nothing is prescribed and the host is not in the loop: every block
of --every steps is ONE native call with the poses recorded on the device.  Prints the height c_z and the velocity v_z of the centre
against time.

    python examples/settling_sphere_ibm_hip.py [--size 32] [--steps 60] [--every 5] [--density 8] [--gravity 2e-4] [--sweeps 2]
    python examples/settling_sphere_ibm_hip.py --size 24 --density 1.15 --virtual-mass 8 --floor --drop 1.1 --gravity 2e-3 --steps 10000 --every 500

The defaults run in seconds.  The coupling is explicit, so the body must be heavy against the fluid it drags along: the marker force
of IBMStepper is the velocity deficit added up over the sweeps that ran, an added mass of about sweeps x (marker area) that has to
stay below the effective mass (density - 1) x volume.  Density 8 with 2 sweeps settles smoothly at the default size; density 2.5 with
4 sweeps oscillates and diverges within ten steps (tests/_ibm_dynamics_ref.py works the figures out).

For a validation run, ten Cate et al. (Phys. Fluids 14 (2002) 4012) measured a nylon sphere, d = 15 mm, rho_p = 1120 kg/m^3, settling
in silicone oil in a 100 x 100 x 160 mm box from 120 mm above the bottom: case E1 rho_f = 970, mu = 0.373 Pa s, Re = 1.5,
u_inf = 0.038 m/s; E2 965 / 0.212 / 4.1 / 0.060; E3 962 / 0.113 / 11.6 / 0.091; E4 960 / 0.058 / 31.9 / 0.128.  Their density ratios
are 1.15 .. 1.17 — BELOW what the explicit scheme alone takes (RigidDynamics.sphere refuses ratios up to 1.2 without a virtual
mass).  --virtual-mass C_v adds the virtual-mass term of Schwarz, Kempe and Froehlich (J. Comput. Phys. 281 (2015) 591), C_v x the
displaced mass, with which such a sphere runs (C_v = 8 in the second line above); nobody has compared a run with their curves yet,
so this example is a demonstration and not a validation.  The box is closed by bounce-back walls.  Without --floor there is no
contact force and the run stops before the sphere comes within two cells of the bottom; with --floor a plane three cells above the
bottom repels the sphere (IBMStepper.set_contact: range 1 cell, wall stiffness --stiffness) and it comes to rest on it, still one
native call per block of steps.  --drop H starts the sphere with its lowest point H cells above that plane."""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import xlb_amd as xlb
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.grid import grid_factory
from xlb_amd.helper.ibm_helper import IBMBody, RigidDynamics, calculate_voronoi_areas, icosphere
from xlb_amd.operator.boundary_condition import FullwayBounceBackBC
from xlb_amd.operator.stepper import IBMStepper

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=32, help="cells along x and y; the box is 1.5 times as high")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--every", type=int, default=5, help="print every so many steps")
ap.add_argument("--density", type=float, default=8.0, help="of the sphere; the fluid's is 1")
ap.add_argument("--gravity", type=float, default=2e-4, help="lattice units, along -z")
ap.add_argument("--viscosity", type=float, default=1.0 / 6.0, help="lattice units (1/6: omega = 1)")
ap.add_argument("--sweeps", type=int, default=2, help="ibm_max_iterations")
ap.add_argument("--relaxation", type=float, default=0.5)
ap.add_argument("--virtual-mass", type=float, default=0.0, help="virtual-mass coefficient C_v (0: none); lets --density go down to just above 1")
ap.add_argument("--floor", action="store_true", help="a contact plane three cells above the bottom that the sphere lands on")
ap.add_argument("--stiffness", type=float, default=1.0, help="wall stiffness of the floor's contact force")
ap.add_argument("--drop", type=float, default=None, help="start with the sphere's lowest point this far above the floor plane")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
lattice = xlb.velocity_set.D3Q19(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

shape = (args.size, args.size, args.size * 3 // 2)
grid = grid_factory(shape)
box = grid.bounding_box_indices()
walls = [sum((box[face][i] for face in ("bottom", "top", "front", "back", "left", "right")), []) for i in range(3)]
walls = np.unique(np.array(walls), axis=-1).tolist()

radius = 0.15 * args.size
centre = np.array([args.size / 2 + 0.3, args.size / 2 + 0.2, shape[2] - 2.0 * radius - 3.0])  # off the lattice on purpose
FLOOR, RANGE = 3.0, 1.0  # the plane keeps the markers' supports (two cells) above the wall cells
if args.drop is not None:
    centre[2] = FLOOR + radius + args.drop
subdivisions = 0
while 4.0 * np.pi * radius**2 / (10 * 4**subdivisions + 2) > 1.0 and subdivisions < 7:
    subdivisions += 1
unit, faces = icosphere(subdivisions)
vertices = (unit * radius + centre).astype(np.float32)
areas = calculate_voronoi_areas(vertices, faces)

stepper = IBMStepper(grid=grid, boundary_conditions=[FullwayBounceBackBC(indices=walls)], collision_type="BGK", ibm_max_iterations=args.sweeps,
                     ibm_tolerance=0.0, ibm_relaxation=args.relaxation)
f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
stepper.markers(vertices, areas, np.zeros_like(vertices))
body = RigidDynamics.sphere(radius, args.density, centre, gravity=(0.0, 0.0, -args.gravity), rotate="locked", virtual_mass_coefficient=args.virtual_mass)
if args.floor:
    weight = -float(body.force[2])
    assert args.stiffness * RANGE**2 > weight, f"--stiffness {args.stiffness} cannot carry the weight {weight:.4g} within the range {RANGE}"
    stepper.set_contact(RANGE, args.stiffness, box=((-np.inf, -np.inf, FLOOR), (np.inf, np.inf, np.inf)))
stepper.set_bodies([IBMBody(markers=slice(0, len(vertices)), dynamics=body, contact_radius=radius if args.floor else None)])
omega = 1.0 / (3.0 * args.viscosity + 0.5)
print(f"box {shape}, sphere radius {radius:.2f} ({len(vertices)} markers) at {centre}, density {args.density}, effective mass {body.mass:.1f}, "
      f"added mass of the coupling about {args.sweeps * float(areas.sum()):.1f}, gravity {args.gravity}, omega {omega:.4f}")

ctx = xlb.default_config.get_context()
t0 = time.perf_counter()
done = 0
print(f"step {done:6d}  c_z {centre[2]:.6f}  v_z {0.0:.6e}")
while done < args.steps:
    n = min(args.every, args.steps - done)
    f_0, f_1, poses = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=done, record_poses=True)
    done += n
    pose = stepper.body_poses()[0]  # (raises if the state stopped being finite)
    print(f"step {done:6d}  c_z {pose[11]:.6f}  v_z {pose[17]:.6e}")
    if not args.floor and pose[11] - radius < 4.0:
        print("the sphere is within two cells of the bottom (there is no contact force): stopping")
        break
ctx.sync()
print(f"{done} steps in {time.perf_counter() - t0:.2f} s; free fall without fluid would have reached v_z = {-args.gravity * done:.6e}")
assert np.isfinite(f_0.numpy()).all()
if args.floor:
    gap, lift = pose[11] - radius - FLOOR, stepper.body_contact_forces()[0, 2]
    print(f"gap above the floor plane {gap:.6f} (contact range {RANGE}), contact force {lift:.6e} against the weight {weight:.6e}, v_z {pose[17]:.6e}")
