#!/usr/bin/env python3
"""Obstacle identification on the HIP backend: recover a hidden solidity field alpha(x) in a 2-D channel from the velocity field after
N steps, by projected gradient descent with the adjoint gradient with respect to geometry (PorousStepper + AdjointStepper.gradient).

    python examples/obstacle_identification_hip.py [--nx 64] [--ny 24] [--steps 40] [--iterations 8] [--reference]

A D2Q9 channel: EquilibriumBC inlet on the left, DoNothingBC outlet on the right, fullway walls above and below, started from the
inlet's uniform flow.  The hidden solidity is a smoothed disc; the target u_target is the bare velocity after N steps with it.  The loss
is L(alpha) = 1/2 |u_N(alpha) - u_target|^2; its gradient dL/dalpha comes from one forward pass and one backward sweep.  Each iteration
tries alpha <- clip(alpha - t dL/dalpha, 0, 1) (the clip is the projection onto [0, 1], on the host) and halves t until the loss falls
(backtracking); an accepted step doubles t for the next iteration.  Prints the loss per iteration and the final L2 distance of alpha
from the hidden field.

``--reference`` runs the same loop on the host through the NumPy restatement tests/_porous_ref.py (no device needed)."""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=64)
ap.add_argument("--ny", type=int, default=24)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--iterations", type=int, default=8)
ap.add_argument("--omega", type=float, default=1.2)
ap.add_argument("--inlet-velocity", type=float, default=0.05)
ap.add_argument("--checkpoint-every", type=int, default=8)
ap.add_argument("--reference", action="store_true", help="the same loop on the host through tests/_porous_ref.py")
args = ap.parse_args()

shape = (args.nx, args.ny)
u_in = (args.inlet_velocity, 0.0)

# the hidden field: a smoothed disc of solidity 0.9 a third of the way down the channel
x, y = np.meshgrid(np.arange(args.nx), np.arange(args.ny), indexing="ij")
radius, width = args.ny / 5.0, 1.5
hidden = 0.9 * 0.5 * (1.0 - np.tanh((np.hypot(x - args.nx / 3.0, y - (args.ny - 1) / 2.0) - radius) / width))
hidden = hidden[None]


def device_problem():
    """(loss(alpha), loss_and_gradient(alpha)) on the device; alpha: a host array (1, nx, ny)"""
    import xlb_amd as xlb
    from xlb_amd import ComputeBackend, PrecisionPolicy
    from xlb_amd.grid import grid_factory
    from xlb_amd.operator.boundary_condition import DoNothingBC, EquilibriumBC, FullwayBounceBackBC
    from xlb_amd.operator.equilibrium import QuadraticEquilibrium
    from xlb_amd.operator.macroscopic import Macroscopic, MacroscopicAdjoint
    from xlb_amd.operator.stepper import AdjointStepper, PorousStepper

    policy = PrecisionPolicy.FP64FP64
    lattice = xlb.velocity_set.D2Q9(precision_policy=policy, compute_backend=ComputeBackend.HIP)
    xlb.init(velocity_set=lattice, default_backend=ComputeBackend.HIP, default_precision_policy=policy)
    grid = grid_factory(shape)
    box, box_ne = grid.bounding_box_indices(), grid.bounding_box_indices(remove_edges=True)
    walls = np.unique(np.concatenate([np.asarray(box[s]) for s in box if s not in ("left", "right")], axis=1), axis=-1).tolist()
    bcs = [FullwayBounceBackBC(indices=walls), EquilibriumBC(rho=1.0, u=u_in, indices=box_ne["left"]), DoNothingBC(indices=box_ne["right"])]
    forward = PorousStepper(grid, boundary_conditions=bcs)
    adjoint = AdjointStepper(forward)
    f_a, f_b, bc_mask, missing_mask = forward.prepare_fields()
    compute = policy.compute_precision
    rho, u, u_bar = grid.create_field(1, dtype=compute), grid.create_field(2, dtype=compute), grid.create_field(2, dtype=compute)
    macroscopic = Macroscopic()
    rho.fill(1.0)
    u.assign(np.broadcast_to(np.array(u_in)[:, None, None], (2,) + shape))
    f_init = QuadraticEquilibrium()(rho, u, grid.create_field(lattice.q, dtype=policy.store_precision))
    alpha = forward.create_solidity()
    forward.set_solidity(alpha)
    state = {}

    def velocity(a):
        alpha.assign(a)
        f_a.copy_from(f_init)
        f, _ = forward.run(f_a, f_b, bc_mask, missing_mask, args.omega, args.steps)
        macroscopic(f, rho, u)
        return u.numpy()

    u_target = velocity(hidden)

    def loss(a):
        return 0.5 * float(np.sum((velocity(a) - u_target) ** 2))

    def cotangent(f_final):
        macroscopic(f_final, rho, u)
        diff = u.numpy() - u_target
        state["loss"] = 0.5 * float(np.sum(diff**2))
        u_bar.assign(diff)
        return MacroscopicAdjoint()(f_final, None, u_bar, adjoint.create_cotangent())

    def loss_and_gradient(a):
        alpha.assign(a)
        lam_0, _, d_alpha = adjoint.gradient(f_init, bc_mask, missing_mask, args.omega, args.steps, cotangent, checkpoint_every=args.checkpoint_every)
        g = d_alpha.numpy()
        lam_0.free()
        d_alpha.free()
        return state["loss"], g

    return loss, loss_and_gradient


def reference_problem():
    """the same two functions through the NumPy restatement"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _adjoint_ref as adj
    import _porous_ref as ref
    from oracle import xlb_numpy as orc

    policy, lat = "FP64FP64", orc.Lattice("D2Q9")
    box, box_ne = orc.bounding_box_indices(shape), orc.bounding_box_indices(shape, remove_edges=True)
    walls = np.unique(np.concatenate([np.asarray(box[s]) for s in box if s not in ("left", "right")], axis=1), axis=-1).tolist()
    bcs = [orc.BC(orc.KIND_FULLWAY_BB, 1, walls), orc.BC(orc.KIND_EQUILIBRIUM, 2, box_ne["left"], rho=1.0, u=u_in),
           orc.BC(orc.KIND_DO_NOTHING, 3, box_ne["right"])]
    bm, mm = orc.build_masks(shape, lat, bcs)
    T = orc.compute_dtype(policy)
    f_init = orc.equilibrium(np.ones((1,) + shape, T), np.broadcast_to(np.array(u_in, T)[:, None, None], (2,) + shape), lat, T)

    def velocity(a):
        return orc.macroscopic(ref.run(f_init, a, bm, mm, bcs, args.omega, lat, args.steps, policy), lat)[1]

    u_target = velocity(hidden)

    def loss(a):
        return 0.5 * float(np.sum((velocity(a) - u_target) ** 2))

    def loss_and_gradient(a):
        state = {}

        def cotangent(f_final):
            diff = orc.macroscopic(f_final, lat)[1] - u_target
            state["loss"] = 0.5 * float(np.sum(diff**2))
            return adj.macroscopic_adjoint(f_final, np.zeros((1,) + shape, T), diff, lat, policy)

        _, _, d_alpha, _ = ref.gradient(f_init, a, bm, mm, bcs, args.omega, lat, args.steps, cotangent, policy)
        return state["loss"], d_alpha

    return loss, loss_and_gradient


loss, loss_and_gradient = reference_problem() if args.reference else device_problem()

alpha = np.zeros_like(hidden)
print(f"{args.nx}x{args.ny} channel, {args.steps} steps, {'host restatement' if args.reference else 'device'}; "
      f"|alpha - hidden| at the start = {np.linalg.norm(alpha - hidden):.6f}")
t = None
first = last = None
for it in range(args.iterations):
    value, g = loss_and_gradient(alpha)
    if first is None:
        first = value
    if t is None:
        t = 0.5 / float(np.abs(g).max())  # the first trial moves the most sensitive cell by 0.5
    accepted = False
    for _ in range(12):
        trial = np.clip(alpha - t * g, 0.0, 1.0)
        trial_value = loss(trial)
        if trial_value < value:
            accepted = True
            break
        t *= 0.5
    print(f"iteration {it}: loss = {value:.12e}, |dL/dalpha| = {np.linalg.norm(g):.6e}, step = {t:.6e}, accepted = {accepted}")
    if not accepted:
        break
    alpha, last = trial, trial_value
    t *= 2.0
print(f"final loss = {(last if last is not None else first):.12e} (first {first:.12e})")
print(f"final |alpha - hidden| = {np.linalg.norm(alpha - hidden):.6f}")
