"""Scalar-transport stepper: the fused fluid step carrying one advected and diffused scalar (a temperature, a concentration, a
tracer), optionally coupled back to the flow by buoyancy.

No counterpart in the reference, which only names the physics (``PhysicsType.ADE``, xlb/physics_type.py); the step is pinned by the
NumPy restatement tests/_scalar_ref.py.

    hot, cold = HalfwayBounceBackBC(indices=box["bottom"]), HalfwayBounceBackBC(indices=box["top"])
    stepper = ScalarTransportStepper(grid, boundary_conditions=[hot, cold],
                                     scalar_boundary_conditions=[ScalarDirichletBC(1.0, on=hot), ScalarDirichletBC(0.0, on=cold)],
                                     collision_type="BGK", buoyancy=(0, 0, g_beta), scalar_reference=0.5)
    f_0, f_1, g_0, g_1, bc_mask, missing_mask = stepper.prepare_fields(scalar=0.5)     # a float or an (nx, ny[, nz]) array
    for i in range(n):
        f_0, f_1, g_0, g_1 = stepper(f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, i)
        f_0, f_1, g_0, g_1 = f_1, f_0, g_1, g_0
    f, f_other, g, g_other = stepper.run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, n)   # native loop, no host wait
    phi = ScalarMoment()(g, phi)

The scalar field ``g`` has cardinality 2 d + 1 in the store dtype and the layout of ``f``: direction 0 is the rest direction, the
others are the lattice's ``main_indices`` in ascending order (D2Q5 inside D2Q9, D3Q7 inside D3Q19 / D3Q27), with the weights
w_0 = 1/4, w_j = 1/8, cs^2 = 1/4 in 3-D and w_0 = 1/3, w_j = 1/6, cs^2 = 1/3 in 2-D.  One kernel (csrc/scalar_step_kernel.hpp)
pulls, updates and stores both fields:

    geq_j = w_j phi (1 + c_j.u / cs^2),    g <- g - omega_scalar (g - geq),    D = cs^2 (1 / omega_scalar - 1/2)

with phi the sum of the post-streaming g and u the velocity of the post-streaming f.  With ``buoyancy`` (or ``force_vector``) the
fluid collides through the exact-difference forced path with the per-cell force ``force_vector + buoyancy (phi - scalar_reference)``;
without them the scalar is passive and the fluid populations are those of IncompressibleNavierStokesStepper bit for bit (the
bit-exact collisions: for fp64 KBC compare with the ``exact_math`` option).  ``prepare_fields`` initialises g_0 = geq(scalar, u(f_0)):
the equilibrium at the initial FLOW, not at rest.

Scalar boundary rules (boundary_condition/scalar_boundary_condition.py) attach to fluid BCs by ``on=``.  Fluid BCs the coupled
kernel supports: EquilibriumBC, HalfwayBounceBackBC (also with a constant wall velocity), FullwayBounceBackBC, DoNothingBC,
ZouHeBC / RegularizedBC with constant values, ExtrapolationOutflowBC.

Limits (NotImplementedError at construction): HybridBC, profile tables and time-dependent walls; fp16 storage; slab-decomposed
fields.  Every call runs its step at once (no pairing of reference-style calls) and the two-step kernel is never used.  Not covered:
conjugate heat transfer, scalar sources, flux walls, the wall-velocity term of anti-bounce-back at moving walls, more than one scalar,
FlowStatistics of phi."""

import numpy as np

from ... import _lib
from ...compute_backend import ComputeBackend
from ..boundary_condition import FullwayBounceBackBC
from ..boundary_condition.scalar_boundary_condition import ScalarBoundaryCondition, ScalarDirichletBC
from ..collision import SmagorinskyLESBGK
from ..operator import Operator
from .nse_stepper import IncompressibleNavierStokesStepper, refuse_regularized, refuse_unsupported


class ScalarTransportStepper(IncompressibleNavierStokesStepper):
    def __init__(self, grid, boundary_conditions=[], scalar_boundary_conditions=[], collision_type="BGK", buoyancy=None, scalar_reference=0.0,
                 force_vector=None):
        refuse_regularized("ScalarTransportStepper", collision_type)
        super().__init__(grid, boundary_conditions, collision_type=collision_type, force_vector=force_vector, backend_config={"lazy_pairs": False})
        vs = self.velocity_set
        refuse_unsupported("ScalarTransportStepper", self.precision_policy, grid, self.boundary_conditions, hybrid="HybridBC is not supported by the coupled kernel")
        self.scalar_boundary_conditions = list(scalar_boundary_conditions)
        seen = set()
        for rule in self.scalar_boundary_conditions:
            if not isinstance(rule, ScalarBoundaryCondition):
                raise ValueError("scalar_boundary_conditions takes ScalarDirichletBC / ScalarAdiabaticBC / ScalarDoNothingBC")
            if not any(rule.on is bc for bc in self.boundary_conditions):
                raise ValueError(f"{type(rule).__name__} attaches to a {type(rule.on).__name__} that is none of this stepper's boundary conditions")
            if rule.on.id in seen:
                raise ValueError(f"two scalar rules attach to the same {type(rule.on).__name__}")
            seen.add(rule.on.id)
            if isinstance(rule, ScalarDirichletBC) and isinstance(rule.on, FullwayBounceBackBC):
                raise ValueError("ScalarDirichletBC cannot attach to a FullwayBounceBackBC: the scalar is bounced fullway there")
        if buoyancy is not None:
            buoyancy = np.asarray(buoyancy, dtype=np.float64)
            if buoyancy.shape != (vs.d,):
                raise AssertionError("Check the dimensions of the input buoyancy!")
        self.buoyancy = buoyancy
        self.scalar_reference = float(scalar_reference)
        self.scalar_q = 2 * vs.d + 1
        self.scalar_directions = np.concatenate([[vs.center_index], np.sort(vs.main_indices)]).astype(np.int64)  # fluid direction of each scalar one
        self._scalar = None

    def _scalar_native(self):
        if self._scalar is None:
            descs = [bc._hip_descriptor() for bc in self.boundary_conditions]
            s = _lib.Scalar(self._ctx, self.velocity_set.hip_id, self.collision.hip_collision_id, self._compute_code, self._store_code, descs)
            s.set_rules([rule._hip_rule() for rule in self.scalar_boundary_conditions])
            coef = self.collision.smagorinsky_coef if isinstance(self.collision, SmagorinskyLESBGK) else 0.17
            s.set_coupling(self._internal3(self.force_vector), self._internal3(self.buoyancy), self.scalar_reference, coef)
            self._scalar = s
        return self._scalar

    def prepare_fields(self, scalar=0.0, initializer=None):
        f_0, f_1, bc_mask, missing_mask = super().prepare_fields(initializer)
        store = self.precision_policy.store_precision
        g_0 = self.grid.create_field(cardinality=self.scalar_q, dtype=store)
        g_1 = self.grid.create_field(cardinality=self.scalar_q, dtype=store)
        if np.ndim(scalar) == 0:
            self._scalar_native().init(f_0, None, float(scalar), g_0)
        else:
            values = np.asarray(scalar, dtype=self.compute_dtype)
            if values.shape != tuple(self.grid.shape):
                raise ValueError(f"scalar must be a number or an array of the grid's shape {tuple(self.grid.shape)}, got {values.shape}")
            phi = self.grid.create_field(cardinality=1, dtype=self.precision_policy.compute_precision)
            phi.assign(values[None])
            self._scalar_native().init(f_0, phi, 0.0, g_0)
            self._ctx.sync()
            phi.free()
        return f_0, f_1, g_0, g_1, bc_mask, missing_mask

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, timestep):
        self._scalar_native().step(f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, timestep)
        return f_0, f_1, g_0, g_1

    def run(self, f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, n_steps, first_timestep=0):
        """``n_steps`` x (step, swap both pairs) in native code, nothing waits for the device; returns (f, f_other, g, g_other) with the
        fields that hold the result first."""
        in_b = self._scalar_native().run(f_0, f_1, g_0, g_1, bc_mask, missing_mask, omega, omega_scalar, first_timestep, n_steps)
        return (f_1, f_0, g_1, g_0) if in_b else (f_0, f_1, g_0, g_1)

    def run_timed(self, *args, **kwargs):
        raise NotImplementedError("ScalarTransportStepper has no run_timed: bracket run() with ctx.sync() and a wall clock")
