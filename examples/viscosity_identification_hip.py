#!/usr/bin/env python3
"""Viscosity identification on the HIP backend: recover the relaxation rate omega of a decaying shear wave from its velocity field
after N steps, by gradient descent with the adjoint gradient (AdjointStepper.gradient, checkpointed).

    python examples/viscosity_identification_hip.py [--n 32] [--steps 100] [--omega-target 1.2] [--omega-start 1.6] [--iterations 8]

A periodic D2Q9 box with u_x = U sin(2 pi y / n).  The target field u_target is the velocity after N steps at omega*; the loss is
L(omega) = 1/2 |u_N(omega) - u_target|^2, its gradient dL/domega comes from one forward pass and one backward sweep, and
omega <- omega - rate * dL/domega.  The wave decays as exp(-nu k^2 t) with nu = (1 / omega - 1/2) / 3, so the loss has one minimum,
at omega*.  Prints omega and the loss per iteration.
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
from xlb_amd.operator.macroscopic import Macroscopic, MacroscopicAdjoint
from xlb_amd.operator.stepper import AdjointStepper, IncompressibleNavierStokesStepper

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=32)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--omega-target", type=float, default=1.2)
ap.add_argument("--omega-start", type=float, default=1.6)
ap.add_argument("--iterations", type=int, default=8)
ap.add_argument("--rate", type=float, default=2.0, help="descent step; the loss' curvature at the default size is about 0.4")
ap.add_argument("--checkpoint-every", type=int, default=10)
args = ap.parse_args()

policy = PrecisionPolicy.FP64FP64
lattice = xlb.velocity_set.D2Q9(precision_policy=policy, compute_backend=ComputeBackend.HIP)
xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)

n = args.n
grid = grid_factory((n, n))
forward = IncompressibleNavierStokesStepper(grid, boundary_conditions=[])
adjoint = AdjointStepper(forward)
f_a, f_b, bc_mask, missing_mask = forward.prepare_fields()
compute = policy.compute_precision
rho, u = grid.create_field(1, dtype=compute), grid.create_field(2, dtype=compute)
macroscopic = Macroscopic()

# the shear wave at equilibrium
_, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
u0 = np.zeros((2, n, n))
u0[0] = 0.05 * np.sin(2 * np.pi * y / n)
rho.fill(1.0)
u.assign(u0)
f_init = QuadraticEquilibrium()(rho, u, grid.create_field(lattice.q, dtype=policy.store_precision))


def velocity_after(omega):
    f_a.copy_from(f_init)
    f, _ = forward.run(f_a, f_b, bc_mask, missing_mask, omega, args.steps)
    macroscopic(f, rho, u)
    return u.numpy()


u_target = velocity_after(args.omega_target)
state = {}


def cotangent(f_final):
    """dL/df_N of L = 1/2 |u_N - u_target|^2: MacroscopicAdjoint of dL/du = u_N - u_target"""
    macroscopic(f_final, rho, u)
    diff = u.numpy() - u_target
    state["loss"] = 0.5 * float(np.sum(diff**2))
    u_bar = grid.create_field(2, dtype=compute)
    u_bar.assign(diff)
    return MacroscopicAdjoint()(f_final, None, u_bar, adjoint.create_cotangent())


omega = args.omega_start
print(f"{n}x{n} shear wave, {args.steps} steps, target omega {args.omega_target}")
for it in range(args.iterations):
    lam_0, d_omega = adjoint.gradient(f_init, bc_mask, missing_mask, omega, args.steps, cotangent, checkpoint_every=args.checkpoint_every)
    lam_0.free()
    print(f"iteration {it}: omega = {omega:.10f}, loss = {state['loss']:.6e}, dL/domega = {d_omega:.6e}")
    omega -= args.rate * d_omega
print(f"final omega = {omega:.10f} (target {args.omega_target}, started at {args.omega_start})")
