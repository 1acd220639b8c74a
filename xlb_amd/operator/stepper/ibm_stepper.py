"""Immersed-boundary stepper: the fused fluid step, then a multi-direct-forcing coupling to Lagrangian markers.

Reference: xlb/operator/stepper/ibm_stepper.py — constructor :28-115, Peskin's 4-point weights :156-178, the sweeps :264-371, the
call :379-476.

    stepper = IBMStepper(grid, boundary_conditions, collision_type="KBC", ibm_max_iterations=4, ibm_tolerance=1e-5)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    for i in range(n):
        f_0, f_1, lag_forces = stepper(f_0, f_1, vertices, areas, velocities, bc_mask, missing_mask, omega, i)
        f_0, f_1 = f_1, f_0

``vertices`` (n, 3), ``areas`` (n,), ``velocities`` (n, 3) are float32 NumPy arrays in lattice units (cell (i, j, k) sits at
(i + 1/2, j + 1/2, k + 1/2)), uploaded by every call that passes them — the footprint of the markers is rebuilt only when the
positions differ from the previous call's.  A body that does not change is better handed over once:

    markers = stepper.markers(vertices, areas, velocities)      # device resident
    stepper(f_0, f_1, markers, None, None, bc_mask, missing_mask, omega, i)
    markers.update(velocities=new_velocities)                   # in place; None keeps an array

One call = one step of the ordinary kernel (never deferred by the pairing of reference-style calls, never the two-step kernel) and
the coupling kernels of csrc/ibm_kernels.hpp on the cells within two cells of a marker.  Nothing in a call waits for the device: the
early exit of the sweep loop is taken by the kernels themselves, ``lag_forces`` is read when somebody asks for its values
(``lag_forces.numpy()``: the forces of the LAST call) and so is ``stepper.ibm_iterations_used``.

3-D lattices, fp32 / fp64 storage, one rank."""

import numpy as np

from ... import _lib
from ...compute_backend import ComputeBackend
from ...precision_policy import Precision
from ..operator import Operator
from .nse_stepper import IncompressibleNavierStokesStepper


class IBMMarkers:
    """The markers of an IBMStepper on the device (there is one set per stepper)."""

    def __init__(self, stepper):
        self._stepper = stepper

    def __len__(self):
        return self._stepper._ibm_native().n

    def update(self, vertices=None, areas=None, velocities=None):
        """Replace any of the three arrays (same number of markers), or all three with a new number of markers."""
        given = [a for a in (vertices, areas, velocities) if a is not None]
        n = len(given[0]) if given else len(self)
        self._stepper._ibm_native().set_markers(n, vertices, areas, velocities)
        return self


class LagrangianForces:
    """``lag_forces`` of the last IBMStepper call, (n, 3) in the compute dtype; read from the device on demand."""

    def __init__(self, stepper):
        self._stepper = stepper

    def numpy(self):
        s = self._stepper
        return s._ibm_native().forces().astype(s.compute_dtype)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)


class IBMStepper(IncompressibleNavierStokesStepper):
    def __init__(self, grid, boundary_conditions=[], collision_type="BGK", use_scoped_timer=False, ibm_max_iterations=4, ibm_tolerance=1e-5,
                 ibm_relaxation=1.0):
        # the pairing of reference-style calls is off: every call runs its step at once
        super().__init__(grid, boundary_conditions, collision_type=collision_type, backend_config={"lazy_pairs": False})
        if self.velocity_set.d != 3:
            raise NotImplementedError("IBMStepper: 2-D grids are not supported (the coupling kernels are written for D3Q19 / D3Q27)")
        if self.precision_policy.store_precision is Precision.FP16:
            raise NotImplementedError(f"IBMStepper: fp16 storage ({self.precision_policy.name}) is not supported; use FP32FP32, FP64FP64 or FP64FP32")
        if getattr(grid, "halo", 0) != 0 or getattr(grid, "n_ranks", 1) != 1:
            raise NotImplementedError("IBMStepper: slab-decomposed fields (ghost planes, several ranks) are not supported")
        self.use_scoped_timer = bool(use_scoped_timer)  # (accepted for the reference's signature; timing is run_timed's job here)
        self.ibm_max_iterations = int(ibm_max_iterations)
        self.ibm_tolerance = float(ibm_tolerance)
        self.ibm_relaxation = float(ibm_relaxation)
        if not 0 <= self.ibm_max_iterations <= 64:
            raise ValueError("ibm_max_iterations must be 0 .. 64")
        if self.ibm_tolerance < 0:
            raise ValueError("ibm_tolerance must not be negative")
        self._ibm = None
        self._markers = IBMMarkers(self)
        self.s_lagr_forces = LagrangianForces(self)

    def _ibm_native(self):
        if self._ibm is None:
            self._ibm = _lib.IBM(self._ctx, self._native_stepper(), self.velocity_set.hip_id, self._compute_code, self._store_code, self.grid.shape,
                                 self.ibm_max_iterations, self.ibm_tolerance, self.ibm_relaxation)
        return self._ibm

    def markers(self, vertices, areas, velocities):
        """Upload a set of markers and return the device-resident object to pass instead of the three arrays."""
        return self._markers.update(vertices, areas, velocities)

    def _set_markers(self, vertices, areas, velocities):
        if isinstance(vertices, IBMMarkers):
            if vertices._stepper is not self:
                raise ValueError("these markers belong to another IBMStepper")
            if areas is not None and not isinstance(areas, IBMMarkers) or velocities is not None and not isinstance(velocities, IBMMarkers):
                vertices.update(None, None if isinstance(areas, IBMMarkers) else areas, None if isinstance(velocities, IBMMarkers) else velocities)
            return
        self._markers.update(vertices, areas, velocities)

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f_0, f_1, vertices, areas, velocities, bc_mask, missing_mask, omega, timestep):
        self._set_markers(vertices, areas, velocities)
        self._stage(timestep, 1)
        self._ibm_native().step(f_0, f_1, bc_mask, missing_mask, omega, timestep)
        return f_0, f_1, self.s_lagr_forces

    def run(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """``n_steps`` x (step with the coupling, swap) in native code with the markers as they are; returns (f_current, f_other)."""
        ibm = self._ibm_native()
        if self._time_dependent_bcs():
            cur, oth = f_0, f_1
            for k in range(int(n_steps)):
                self._stage(first_timestep + k, 1)
                ibm.step(cur, oth, bc_mask, missing_mask, omega, first_timestep + k)
                cur, oth = oth, cur
            return cur, oth
        in_b = ibm.run(f_0, f_1, bc_mask, missing_mask, omega, first_timestep, n_steps)
        return (f_1, f_0) if in_b else (f_0, f_1)

    def run_timed(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """As :meth:`run`; also returns the wall-clock milliseconds between two synchronisations."""
        import time

        self._ctx.sync()
        t0 = time.perf_counter()
        out = self.run(f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep)
        self._ctx.sync()
        return out, (time.perf_counter() - t0) * 1e3

    @property
    def ibm_iterations_used(self):
        """Sweeps the last call ran (read from the device now)."""
        return self._ibm_native().iterations()

    def ibm_footprint(self):
        """Linear indices ((x * ny + y) * nz + z) of the cells the coupling works on."""
        return self._ibm_native().footprint()
