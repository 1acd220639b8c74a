#!/usr/bin/env python3
"""Body-force driven channel with on-device statistics — the set-up of examples/turbulent_channel_3d_hip.py (D3Q27 / KBC, exact-difference
body force, RegularizedBC("velocity", 0) walls on the two z faces, periodic in x and y), sampled every few steps by FlowStatistics with
keep_axes=(2,): the time- and plane-averaged profile <u_x>(z), the friction velocity and the Reynolds stresses come out of running sums
kept on the device, no field is ever downloaded and the loop never waits for the device between two reports.

    python examples/channel_statistics_hip.py [--h 32] [--re-tau 180] [--steps 4000] [--every 10] [--spin-up 1000]
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
from xlb_amd.operator.boundary_condition import RegularizedBC
from xlb_amd.operator.equilibrium import QuadraticEquilibrium
from xlb_amd.operator.postprocess import FlowStatistics
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper
from xlb_amd.precision_policy import Precision

ap = argparse.ArgumentParser()
ap.add_argument("--h", type=int, default=32, help="channel half width in cells; the box is 6h x 3h x 2h")
ap.add_argument("--re-tau", type=float, default=180.0)
ap.add_argument("--u-tau", type=float, default=0.004)
ap.add_argument("--steps", type=int, default=4000)
ap.add_argument("--every", type=int, default=10, help="steps between two samples")
ap.add_argument("--spin-up", type=int, default=1000, help="steps before the first sample")
args = ap.parse_args()

policy = PrecisionPolicy.FP32FP32
lattice = xlb.velocity_set.D3Q27(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

h = args.h
shape = (6 * h, 3 * h, 2 * h)
grid = grid_factory(shape)
visc = args.u_tau * h / args.re_tau
omega = 1.0 / (3.0 * visc + 0.5)
force = (args.re_tau * visc) ** 2 / h**3

box = grid.bounding_box_indices()
walls = [box["bottom"][i] + box["top"][i] for i in range(3)]
bc_walls = RegularizedBC("velocity", prescribed_value=(0.0, 0.0, 0.0), indices=walls)
stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[bc_walls], collision_type="KBC", force_vector=(force, 0.0, 0.0))
f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()

# initial field: log-law mean + a sinusoidal perturbation that trips the transition, as an equilibrium
x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
zplus = np.minimum(z + 0.5, 2 * h - 0.5 - z) * args.u_tau / visc
u0 = np.zeros((3,) + shape)
u0[0] = args.u_tau * (np.log(np.maximum(zplus, 1.0)) / 0.41 + 5.5)
amp = 0.1 * u0[0].max()
u0[0] += amp * np.cos(2 * np.pi * y / shape[1] * 3) * np.sin(np.pi * z / shape[2])
u0[1] += amp * np.sin(2 * np.pi * x / shape[0] * 4) * np.sin(np.pi * z / shape[2])
u0[2] += 0.5 * amp * np.sin(2 * np.pi * x / shape[0] * 4) * np.cos(2 * np.pi * y / shape[1] * 3) * np.sin(np.pi * z / shape[2]) ** 2
rho0 = grid.create_field(1, dtype=Precision.FP32, fill_value=1.0)
u_init = grid.create_field(3, dtype=Precision.FP32)
u_init.assign(u0.astype(np.float32))
f_0 = QuadraticEquilibrium()(rho0, u_init, f_0)
print(f"grid {shape}, Re_tau {args.re_tau}, u_tau {args.u_tau}, viscosity {visc:.3e}, omega {omega:.4f}, body force {force:.3e}")

# the wall cells carry the boundary condition's id: they are sampled like every other fluid cell (nothing here is solid)
stats = FlowStatistics(grid, keep_axes=(2,))
ctx = xlb.default_config.get_context()
t0 = time.perf_counter()
done = 0
spin_up = min(args.spin_up, args.steps // 2)
f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, spin_up)
done = spin_up
next_report = done + 1000
while done < args.steps:
    n = min(args.every, args.steps - done)
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, first_timestep=done)
    stats.sample(f_0, bc_mask)  # enqueued behind the steps; the host runs ahead
    done += n
    if done >= next_report or done == args.steps:
        r = stats.result()  # the only synchronisation
        mean = r["u"][0]
        u_tau_now = np.sqrt(visc * abs(mean[1] - mean[0]))  # wall shear from the first two cell centres
        print(f"step {done}: {r['samples']} samples, bulk velocity {mean.mean():.5f}, centre-line {mean[h]:.5f}, u_tau from the wall gradient "
              f"{u_tau_now:.5f} (target {args.u_tau}), largest |u| of the last sample {np.sqrt(r['max_u2']):.4f}")
        next_report += 1000
ctx.sync()
dt = time.perf_counter() - t0

r = stats.result()
mean, stress = r["u"][0], stats.reynolds_stress(r)
uu, uw = stress[0], stress[2]  # <u'u'>, <u'w'> (x streamwise, z wall-normal)
print("   z+      <u>/u_tau   <u'u'>/u_tau^2   <u'w'>/u_tau^2")
for k in sorted(set(list(range(0, h, max(1, h // 8))) + [h - 1])):
    print(f"{(k + 0.5) * args.u_tau / visc:7.1f} {mean[k] / args.u_tau:12.3f} {uu[k] / args.u_tau**2:14.3f} {uw[k] / args.u_tau**2:16.3f}")
peak = int(np.argmax(uu[:h]))
print(f"peak of <u'u'>: {uu[peak] / args.u_tau**2:.3f} u_tau^2 at z+ = {(peak + 0.5) * args.u_tau / visc:.1f}; "
      f"u_tau from the mean profile {np.sqrt(visc * abs(mean[1] - mean[0])):.5f} (target {args.u_tau})")
print(f"{args.steps} steps and {r['samples']} samples in {dt:.2f} s: {np.prod(shape) * args.steps / dt / 1e6:.0f} MLUPS (incl. the statistics)")
# the watchdog stayed clean: every sampled cell finite in every sample, velocities far below the lattice's speed of sound
assert r["nonfinite_total"] == 0 and r["max_u2"] < 0.3**2, (r["nonfinite_total"], r["max_u2"])
assert np.isfinite(mean).all() and mean[h] > 0.0 and r["samples"] > 0
