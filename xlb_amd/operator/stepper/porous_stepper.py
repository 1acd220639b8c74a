"""Porous stepper: the fused BGK step with geometry as a continuous per-cell field, for gradients with respect to geometry.

Each cell carries a solidity ``alpha(x)`` in [0, 1]: 0 is fluid, 1 relaxes the cell towards rest (after Pingen, Evgrafov and Maute
2007).  The step is the fused BGK step with the equilibrium taken at the damped velocity:

    rho, u  = moments(f*)
    ut      = (1 - alpha) u
    f_out_l = f*_l - omega (f*_l - feq_l(rho, ut))

Mass is conserved; momentum leaves at the rate omega alpha rho u per step.  With ``alpha == 0`` the step is the plain BGK step bit for
bit.  Values of alpha outside [0, 1] are the caller's business: nothing checks them, neither here nor on the device (an optimiser
clips or projects on the host).

    forward = PorousStepper(grid, boundary_conditions=[inlet, outlet, walls])
    f_0, f_1, bc_mask, missing_mask = forward.prepare_fields()
    alpha = forward.create_solidity()              # one value per cell, the compute dtype
    alpha.assign(values[None])
    forward.set_solidity(alpha)                    # bound by reference: later assigns to the field are seen by the next step
    f, other = forward.run(f_0, f_1, bc_mask, missing_mask, omega, n_steps)

    adjoint = AdjointStepper(forward)
    lam_0, dL_domega, dL_dalpha = adjoint.gradient(f_init, bc_mask, missing_mask, omega, n_steps, cotangent)   # dL_dalpha: an fp64 field

The device code is csrc/porous_kernels.hpp (the cell rules, with the derivation) and csrc/porous_step_kernel.hpp, pinned by the NumPy
restatement tests/_porous_ref.py.  ``macroscopic`` is the plain operator: the bare velocity u, not the damped one.

Scope: BGK; D2Q9, D3Q19, D3Q27; FP32FP32, FP64FP64, FP64FP32; periodic edges, EquilibriumBC, HalfwayBounceBackBC (a constant wall
velocity or none), FullwayBounceBackBC, DoNothingBC; single rank.  Refused at construction: every other collision, a force vector,
every other boundary condition, profiles, fp16 storage, slab-decomposed fields."""

import time

from ... import _lib
from ...compute_backend import ComputeBackend
from ..boundary_condition import DoNothingBC, EquilibriumBC, FullwayBounceBackBC, HalfwayBounceBackBC
from ..operator import Operator
from .nse_stepper import IncompressibleNavierStokesStepper, refuse_regularized, refuse_unsupported


class PorousStepper(IncompressibleNavierStokesStepper):
    def __init__(self, grid, boundary_conditions=[], collision_type="BGK"):
        refuse_regularized("PorousStepper", collision_type)
        if collision_type != "BGK":
            raise NotImplementedError(f"PorousStepper: collision_type {collision_type!r} is not supported; the porous step is built for BGK")
        super().__init__(grid, boundary_conditions, collision_type="BGK", backend_config={"lazy_pairs": False})

        def known_kinds(bc):
            if type(bc) not in (EquilibriumBC, HalfwayBounceBackBC, FullwayBounceBackBC, DoNothingBC):
                raise NotImplementedError(f"PorousStepper: {type(bc).__name__} is not supported (EquilibriumBC, HalfwayBounceBackBC, "
                                          "FullwayBounceBackBC and DoNothingBC only)")

        refuse_unsupported("PorousStepper", self.precision_policy, grid, self.boundary_conditions, also=known_kinds)
        self._porous = None
        self._solidity = None

    def _porous_native(self):
        if self._porous is None:
            descs = [bc._hip_descriptor() for bc in self.boundary_conditions]
            self._porous = _lib.Porous(self._ctx, self.velocity_set.hip_id, self._compute_code, self._store_code, descs)
        return self._porous

    def create_solidity(self, fill_value=0.0):
        """A solidity field: one value per cell, the compute dtype"""
        return self.grid.create_field(cardinality=1, dtype=self.precision_policy.compute_precision, fill_value=float(fill_value))

    def set_solidity(self, field):
        """Bind ``field`` (made by ``create_solidity``) as alpha: by reference, so what is assigned to it later is what the next step
        reads.  The stepper keeps it alive; an explicit ``field.free()`` while it is bound leaves the native object with a dangling
        address (undefined behaviour on the next step): bind another field first."""
        if not isinstance(field, _lib.Field):
            raise TypeError("PorousStepper.set_solidity takes a field made by create_solidity()")
        compute = self.precision_policy.compute_precision
        if field.dtype_code != compute.hip_dtype:
            raise ValueError(f"PorousStepper: the solidity field must have the compute dtype {compute.name}, got {field.dtype}")
        if field.cardinality != 1 or tuple(field.grid_shape) != tuple(self.grid.local_shape) or field.halo != 0:
            raise ValueError(f"PorousStepper: the solidity field must have shape {(1,) + tuple(self.grid.local_shape)} and no ghost planes, "
                             f"got {field.shape}")
        if field.ctx is not self._ctx:
            raise ValueError("PorousStepper: the solidity field belongs to another context than this stepper's grid")
        self._porous_native().set_solidity(field)
        self._solidity = field

    @property
    def solidity(self):
        return self._solidity

    def _bound(self):
        if self._solidity is None:
            raise RuntimeError("PorousStepper: no solidity field is bound; call set_solidity(create_solidity()) before stepping")
        return self._porous_native()

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f_0, f_1, bc_mask, missing_mask, omega, timestep):
        self._bound().step(f_0, f_1, bc_mask, missing_mask, omega, timestep)
        return f_0, f_1

    def run(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """``n_steps`` x (step, swap) in native code, nothing waits for the device; returns (f_current, f_other)."""
        in_b = self._bound().run(f_0, f_1, bc_mask, missing_mask, omega, first_timestep, n_steps)
        return (f_1, f_0) if in_b else (f_0, f_1)

    def run_timed(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """As :meth:`run`; also returns the milliseconds of the wall clock between two synchronisations."""
        self._bound()
        self._ctx.sync()
        t0 = time.perf_counter()
        out = self.run(f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep)
        self._ctx.sync()
        return out, (time.perf_counter() - t0) * 1e3
