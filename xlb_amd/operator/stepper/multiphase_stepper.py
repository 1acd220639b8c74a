"""Multiphase stepper: single-component Shan-Chen pseudopotential flow (liquid and vapour of one fluid, droplets, films, wetting).

No counterpart in the reference; the step is pinned by the NumPy restatement tests/_multiphase_ref.py.

    bottom, top = HalfwayBounceBackBC(indices=box["bottom"]), HalfwayBounceBackBC(indices=box["top"])
    stepper = MultiphaseStepper(grid, boundary_conditions=[bottom, top], pseudopotential=ShanChenExponential(G=-5.5),
                                wall_density={bottom: 1.2})
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields(density=rho0)          # a float or an array of the grid's shape
    for i in range(n):
        f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, omega, i)
        f_0, f_1 = f_1, f_0
    f, f_other = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n)             # native loop, no host wait
    rho, u = stepper.macroscopic(f, bc_mask, missing_mask)

On the post-streaming populations of every cell (pull, then the streaming-step boundary rules):

    psi = Psi(rho),    F_a = -G psi(x) sum_i w_i psi(x + c_i) c_ai,    BGK with the exact-difference acceleration force_vector + F / rho

with the fluid lattice's own weights, so that the bulk pressure is  p = cs^2 rho + (G cs^2 / 2) psi^2  on D2Q9, D3Q19 and D3Q27.  A
neighbour behind a missing direction counts with Psi(wall_density) of the cell's own boundary condition: a wall density near the
liquid's wets the wall, one near the vapour's repels the liquid.  Fullway bounce-back cells and solid cells (bc id 255 of a mesh
masker) carry their Psi(wall_density) themselves and feel no force.

The force at a cell needs psi of the SAME step's post-streaming density at its neighbours, so a step is two kernels
(csrc/multiphase_step_kernel.hpp): one stores psi, the next pulls again, reads the neighbours' psi and collides.  Fusing them would
mean a force from the previous step's density — a different (lagged) scheme that is not built.

The stored populations are post-collision; their bare first moment is not the physical velocity at an interface.
``macroscopic`` gives rho and u = u_bare + F / (2 rho) of the post-streaming state, ``pseudopotential`` and ``interaction_force`` the
intermediates psi and F (without ``force_vector``).

Pseudopotentials: ``ShanChenExponential(G, rho0)``  psi = rho0 (1 - exp(-rho / rho0));  ``ShanChenDensity(G)``  psi = rho (no phase
separation by itself: the vehicle of the bit-exact tests);  ``CarnahanStarling(T, a, b, R)``  psi = sqrt(2 (p_CS - cs^2 rho) / (G cs^2))
with G = -1 (Yuan and Schaefer 2006), critical temperature 0.3773 a / (b R).

Supported: BGK; D2Q9, D3Q19, D3Q27; FP32FP32, FP64FP64, FP64FP32; periodic edges, HalfwayBounceBackBC (no or a constant wall velocity),
FullwayBounceBackBC, solid cells of a mesh masker; one rank.  Refused at construction: KBC and Smagorinsky, fp16 storage, slab grids,
EquilibriumBC / DoNothingBC / ZouHeBC / RegularizedBC / ExtrapolationOutflowBC (their missing directions have no agreed neighbour
psi), HybridBC, profiles and time-dependent walls, a wall density for a BC that is not this stepper's.  Every call runs its step at once
(no pairing of reference-style calls) and the two-step kernel is never used."""

import numpy as np

from ... import _lib
from ...cell_type import BC_SOLID
from ...compute_backend import ComputeBackend
from ...helper.initializers import initialize_eq
from ..boundary_condition import FullwayBounceBackBC, HalfwayBounceBackBC
from ..boundary_condition.boundary_condition import BoundaryCondition
from ..operator import Operator
from .nse_stepper import IncompressibleNavierStokesStepper, refuse_unsupported

CS2 = 1.0 / 3.0


class Pseudopotential:
    """Psi(rho) of a Shan-Chen model.  ``psi(rho)`` evaluates it in rho's dtype with the device's operation order (the wall table is
    made with it); ``pressure(rho)`` is the bulk equation of state cs^2 rho + (G cs^2 / 2) psi^2."""

    form = None
    G = None

    def parameters(self):
        return []

    def psi(self, rho):
        raise NotImplementedError

    def pressure(self, rho):
        rho = np.asarray(rho, dtype=np.float64)
        return CS2 * rho + 0.5 * self.G * CS2 * self.psi(rho) ** 2


class ShanChenExponential(Pseudopotential):
    form = _lib.Multiphase.EXPONENTIAL

    def __init__(self, G, rho0=1.0):
        self.G, self.rho0 = float(G), float(rho0)
        if not self.rho0 > 0.0:
            raise ValueError(f"ShanChenExponential: rho0 must be positive, got {rho0}")

    def parameters(self):
        return [self.rho0]

    def psi(self, rho):
        rho = np.asarray(rho)
        T = rho.dtype.type
        return T(self.rho0) * (T(1) - np.exp(-(rho / T(self.rho0))))


class ShanChenDensity(Pseudopotential):
    form = _lib.Multiphase.DENSITY

    def __init__(self, G):
        self.G = float(G)

    def psi(self, rho):
        return np.asarray(rho).copy()


class CarnahanStarling(Pseudopotential):
    form = _lib.Multiphase.CARNAHAN_STARLING
    G = -1.0

    def __init__(self, T, a=1.0, b=4.0, R=1.0):
        self.T, self.a, self.b, self.R = float(T), float(a), float(b), float(R)

    @property
    def critical_temperature(self):
        return 0.3773 * self.a / (self.b * self.R)

    def parameters(self):
        return [self.T, self.a, self.b, self.R]

    def eos(self, rho):
        """the Carnahan-Starling pressure itself, in rho's dtype and the device's operation order"""
        rho = np.asarray(rho)
        T = rho.dtype.type
        eta = (T(self.b) * rho) / T(4)
        e2 = eta * eta
        e3 = e2 * eta
        num = ((T(1) + eta) + e2) - e3
        om = T(1) - eta
        den = (om * om) * om
        return (((rho * T(self.R)) * T(self.T)) * num) / den - (T(self.a) * rho) * rho

    def psi(self, rho):
        rho = np.asarray(rho)
        T = rho.dtype.type
        cs2 = T(1.0 / 3.0)
        with np.errstate(invalid="ignore"):
            return np.sqrt((T(2) * (self.eos(rho) - cs2 * rho)) / (T(-1) * cs2))


class MultiphaseStepper(IncompressibleNavierStokesStepper):
    def __init__(self, grid, boundary_conditions=[], pseudopotential=None, wall_density=None, force_vector=None, collision_type="BGK"):
        if collision_type != "BGK":
            raise NotImplementedError(f"MultiphaseStepper: collision_type {collision_type!r} is not supported; the Shan-Chen step is built for BGK only "
                                      "(no KBC, no SmagorinskyLESBGK)")
        if not isinstance(pseudopotential, Pseudopotential):
            raise ValueError("MultiphaseStepper: pseudopotential takes ShanChenExponential, ShanChenDensity or CarnahanStarling")
        super().__init__(grid, boundary_conditions, collision_type="BGK", force_vector=force_vector, backend_config={"lazy_pairs": False})
        del self.macroscopic  # (the fluid stepper's bare-moment operator; here macroscopic() is the method below)

        def walls_only(bc):
            if not isinstance(bc, (HalfwayBounceBackBC, FullwayBounceBackBC)):
                raise NotImplementedError(f"MultiphaseStepper: {type(bc).__name__} is not supported (HalfwayBounceBackBC and FullwayBounceBackBC only): "
                                          "its missing directions have no agreed neighbour pseudopotential")

        refuse_unsupported("MultiphaseStepper", self.precision_policy, grid, self.boundary_conditions, also=walls_only)
        self.model = pseudopotential
        self.wall_density = self._wall_table(wall_density)
        self._multiphase = None

    def _wall_table(self, wall_density):
        """{bc id: rho_w}; one number stands for every BC and the solid cells, a dict names BCs (or "solid" / 255); the rest is 0"""
        ids = [bc.id for bc in self.boundary_conditions]
        if wall_density is None:
            return {}
        if np.ndim(wall_density) == 0 and not isinstance(wall_density, dict):
            table = {i: float(wall_density) for i in ids + [BC_SOLID]}
        else:
            table = {}
            for key, value in dict(wall_density).items():
                if isinstance(key, BoundaryCondition):
                    if not any(key is bc for bc in self.boundary_conditions):
                        raise ValueError(f"wall_density names a {type(key).__name__} that is none of this stepper's boundary conditions")
                    table[key.id] = float(value)
                elif key == "solid" or key == BC_SOLID:
                    table[BC_SOLID] = float(value)
                else:
                    raise ValueError(f"wall_density keys are boundary conditions of this stepper or 'solid', got {key!r}")
        for i, value in table.items():
            if not (np.isfinite(value) and value >= 0.0):
                raise ValueError(f"wall_density of bc id {i} must be a finite density >= 0, got {value}")
        return table

    def wall_psi(self):
        """{bc id: Psi(rho_w)} in the compute dtype: the bits of the device's table"""
        T = self.compute_dtype
        with np.errstate(all="ignore"):
            return {i: self.model.psi(np.array(rho_w, dtype=T))[()] for i, rho_w in self.wall_density.items()}

    def _multiphase_native(self):
        if self._multiphase is None:
            descs = [bc._hip_descriptor() for bc in self.boundary_conditions]
            m = _lib.Multiphase(self._ctx, self.velocity_set.hip_id, self._compute_code, self._store_code, descs)
            pp = self.model
            m.set_model(pp.form, pp.G, pp.parameters(), self._internal3(self.force_vector))
            psi_w = self.wall_psi()
            m.set_wall_density([(i, rho_w, float(psi_w[i])) for i, rho_w in self.wall_density.items()])
            self._multiphase = m
        return self._multiphase

    def prepare_fields(self, density=1.0, initializer=None):
        """f_0 = feq(density, u = 0); ``density``: a float or an array of the grid's shape"""
        f_0, f_1, bc_mask, missing_mask = super().prepare_fields(initializer=(lambda bc_mask, f_0: f_0) if initializer is None else initializer)
        if initializer is None:
            compute = self.precision_policy.compute_precision
            if np.ndim(density) == 0:
                rho = self.grid.create_field(cardinality=1, fill_value=float(density), dtype=compute)
            else:
                values = np.asarray(density, dtype=self.compute_dtype)
                if values.shape != tuple(self.grid.shape):
                    raise ValueError(f"density must be a number or an array of the grid's shape {tuple(self.grid.shape)}, got {values.shape}")
                rho = self.grid.create_field(cardinality=1, dtype=compute)
                rho.assign(values[None])
            f_0 = initialize_eq(f_0, self.grid, self.velocity_set, self.precision_policy, self.compute_backend, rho=rho)
            self._ctx.sync()
            rho.free()
        return f_0, f_1, bc_mask, missing_mask

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f_0, f_1, bc_mask, missing_mask, omega, timestep):
        self._multiphase_native().step(f_0, f_1, bc_mask, missing_mask, omega, timestep)
        return f_0, f_1

    def run(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """``n_steps`` x (step, swap) in native code, nothing waits for the device; returns (f, f_other) with the field that holds the
        result first."""
        in_b = self._multiphase_native().run(f_0, f_1, bc_mask, missing_mask, omega, first_timestep, n_steps)
        return (f_1, f_0) if in_b else (f_0, f_1)

    def run_timed(self, *args, **kwargs):
        raise NotImplementedError("MultiphaseStepper has no run_timed: bracket run() with ctx.sync() and a wall clock")

    def _output(self, cardinality):
        return self.grid.create_field(cardinality=cardinality, dtype=self.precision_policy.compute_precision)

    def pseudopotential(self, f, bc_mask, missing_mask):
        """psi = Psi(rho) of the post-streaming state of the stored field ``f`` (the wall value at fullway and solid cells)"""
        psi = self._output(1)
        self._multiphase_native().psi(f, bc_mask, missing_mask, psi)
        return psi

    def interaction_force(self, f, bc_mask, missing_mask):
        """F of the post-streaming state of the stored field ``f``, without ``force_vector``, the lattice's d components"""
        force = self._output(self.velocity_set.d)
        self._multiphase_native().force(f, bc_mask, missing_mask, force)
        return force

    def macroscopic(self, f, bc_mask, missing_mask):
        """rho and the physical velocity u = u_bare + F / (2 rho) of the post-streaming state of the stored field ``f``"""
        rho, u = self._output(1), self._output(self.velocity_set.d)
        self._multiphase_native().macroscopic(f, bc_mask, missing_mask, rho, u)
        return rho, u
