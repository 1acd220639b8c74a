"""Multicomponent stepper: two immiscible fluids A and B by Shan-Chen coupling (oil and water in a pore space, a droplet of one liquid
in another, layered flow, wetting of a solid by one fluid of a pair).

No counterpart in the reference; the step is pinned by the NumPy restatement tests/_multicomponent_ref.py.

    bottom = HalfwayBounceBackBC(indices=box["bottom"])
    stepper = MulticomponentStepper(grid, boundary_conditions=[bottom], interaction=ShanChenMixture(G_AB=2.4),
                                    wall_density={bottom: (1.05, 0.01), "solid": (0.01, 1.05)})
    fA_0, fA_1, fB_0, fB_1, bc_mask, missing_mask = stepper.prepare_fields(density=(rho_A, rho_B))   # numbers or arrays of the grid's shape
    for i in range(n):
        fA_0, fA_1, fB_0, fB_1 = stepper(fA_0, fA_1, fB_0, fB_1, bc_mask, missing_mask, (omega_A, omega_B), i)
        fA_0, fA_1, fB_0, fB_1 = fA_1, fA_0, fB_1, fB_0
    fA, fA_other, fB, fB_other = stepper.run(fA_0, fA_1, fB_0, fB_1, bc_mask, missing_mask, (omega_A, omega_B), n)   # native loop, no host wait
    rho_A, rho_B, u = stepper.macroscopic(fA, fB, bc_mask, missing_mask)
    F_A, F_B = stepper.interaction_force(fA, fB, bc_mask, missing_mask)

Each component s has populations f^s on the grid's lattice and a relaxation rate omega_s (a single omega stands for both).  On the
post-streaming populations of every cell (pull, then the streaming-step boundary rules, per component):

    u'   = (omega_A rho_A u_A + omega_B rho_B u_B) / (omega_A rho_A + omega_B rho_B)
    F^A  = -rho_A(x) sum_i w_i (G_AA rho_A + G_AB rho_B)(x + c_i) c_i,      F^B = -rho_B(x) sum_i w_i (G_AB rho_A + G_BB rho_B)(x + c_i) c_i
    f^s <- BGK towards feq(rho_s, u') with the exact-difference acceleration force_vector + F^s / rho_s

with the lattice's own weights, so that the bulk pressure is  cs^2 (rho_A + rho_B) + cs^2 (G_AA rho_A^2 / 2 + G_AB rho_A rho_B +
G_BB rho_B^2 / 2)  on D2Q9, D3Q19 and D3Q27.  A neighbour behind a missing direction counts with the pair wall_density of the cell's own
boundary condition: a pair near (rho_A, 0) makes the wall A-wetting.  Fullway bounce-back cells and solid cells (bc id 255 of a mesh
masker) carry their pair themselves and feel no force.

The forces need both densities of the SAME step's post-streaming state at the neighbours, so a step is two kernels
(csrc/multicomponent_step_kernel.hpp): one stores rho_A and rho_B, the next pulls again, reads both stencils and collides both sets.

The stored populations are post-collision.  ``macroscopic`` gives rho_A, rho_B and the barycentric velocity
u = (rho_A u_A + rho_B u_B + (F^A + F^B) / 2) / (rho_A + rho_B) of the post-streaming state, ``densities`` what the force reads (the wall
pair at wall cells), ``interaction_force`` F^A and F^B (without ``force_vector``).

Supported: BGK; D2Q9, D3Q19, D3Q27; FP32FP32, FP64FP64, FP64FP32; periodic edges, resting HalfwayBounceBackBC, FullwayBounceBackBC, solid
cells of a mesh masker; one rank.  Refused at construction: other collisions, fp16 storage, slab grids, every boundary condition that
MultiphaseStepper refuses, a halfway wall with a wall velocity (its constant 6 w (c.u_w) assumes density 1 and would inject the wrong
momentum into a component of density 0.01), a wall density for a BC that is not this stepper's; in ``prepare_fields`` a non-positive
density (the scheme divides by rho_s)."""

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


class ShanChenMixture:
    """The interaction strengths of a pair of components with psi_s = rho_s: G_AB > 0 separates them (beyond G_AB rho of about 1),
    G_AA and G_BB act inside each.  ``pressure(rho_A, rho_B)`` is the bulk equation of state."""

    def __init__(self, G_AB, G_AA=0.0, G_BB=0.0):
        self.G_AB, self.G_AA, self.G_BB = float(G_AB), float(G_AA), float(G_BB)
        if not all(np.isfinite(g) for g in (self.G_AB, self.G_AA, self.G_BB)):
            raise ValueError("ShanChenMixture: the interaction strengths must be finite")

    def pressure(self, rho_a, rho_b):
        a, b = np.asarray(rho_a, dtype=np.float64), np.asarray(rho_b, dtype=np.float64)
        return CS2 * (a + b) + CS2 * (0.5 * self.G_AA * a * a + self.G_AB * a * b + 0.5 * self.G_BB * b * b)


class MulticomponentStepper(IncompressibleNavierStokesStepper):
    def __init__(self, grid, boundary_conditions=[], interaction=None, wall_density=None, force_vector=None, collision_type="BGK"):
        if collision_type != "BGK":
            raise NotImplementedError(f"MulticomponentStepper: collision_type {collision_type!r} is not supported; the two-component step is built "
                                      "for BGK only")
        if not isinstance(interaction, ShanChenMixture):
            raise ValueError("MulticomponentStepper: interaction takes a ShanChenMixture")
        super().__init__(grid, boundary_conditions, collision_type="BGK", force_vector=force_vector, backend_config={"lazy_pairs": False})
        del self.macroscopic  # (the fluid stepper's bare-moment operator; here macroscopic() is the method below)

        def resting_walls_only(bc):
            if not isinstance(bc, (HalfwayBounceBackBC, FullwayBounceBackBC)):
                raise NotImplementedError(f"MulticomponentStepper: {type(bc).__name__} is not supported (HalfwayBounceBackBC and FullwayBounceBackBC "
                                          "only): its missing directions have no agreed neighbour density")
            if isinstance(bc, HalfwayBounceBackBC) and np.any(bc.prescribed_value != 0.0):
                raise NotImplementedError("MulticomponentStepper: a HalfwayBounceBackBC with a wall velocity is not supported: its constant "
                                          "6 w (c.u_w) assumes density 1 and would inject the wrong momentum into a component of another density")

        refuse_unsupported("MulticomponentStepper", self.precision_policy, grid, self.boundary_conditions, also=resting_walls_only)
        self.model = interaction
        self.wall_density = self._wall_table(wall_density)
        self._native = None

    def _wall_table(self, wall_density):
        """{bc id: (rho_w of A, rho_w of B)}; a dict names BCs (or "solid" / 255); the rest is (0, 0)"""
        table = {}
        for key, value in dict(wall_density or {}).items():
            if np.ndim(value) != 1 or len(value) != 2:
                raise ValueError(f"wall_density values are pairs (rho_w of A, rho_w of B), got {value!r}")
            pair = (float(value[0]), float(value[1]))
            if isinstance(key, BoundaryCondition):
                if not any(key is bc for bc in self.boundary_conditions):
                    raise ValueError(f"wall_density names a {type(key).__name__} that is none of this stepper's boundary conditions")
                table[key.id] = pair
            elif key == "solid" or key == BC_SOLID:
                table[BC_SOLID] = pair
            else:
                raise ValueError(f"wall_density keys are boundary conditions of this stepper or 'solid', got {key!r}")
        for i, pair in table.items():
            if not all(np.isfinite(v) and v >= 0.0 for v in pair):
                raise ValueError(f"wall_density of bc id {i} must be two finite densities >= 0, got {pair}")
        return table

    def _multicomponent_native(self):
        if self._native is None:
            descs = [bc._hip_descriptor() for bc in self.boundary_conditions]
            m = _lib.Multicomponent(self._ctx, self.velocity_set.hip_id, self._compute_code, self._store_code, descs)
            mix = self.model
            m.set_model(mix.G_AA, mix.G_AB, mix.G_BB, self._internal3(self.force_vector))
            m.set_wall_density([(i, a, b) for i, (a, b) in self.wall_density.items()])
            self._native = m
        return self._native

    @staticmethod
    def _omegas(omega):
        if np.ndim(omega) == 0:
            return float(omega), float(omega)
        omega_a, omega_b = omega
        return float(omega_a), float(omega_b)

    def _density_field(self, density, name):
        compute = self.precision_policy.compute_precision
        if np.ndim(density) == 0:
            if not float(density) > 0.0:
                raise ValueError(f"prepare_fields: the density of component {name} must be positive (the scheme divides by it), got {density}")
            return self.grid.create_field(cardinality=1, fill_value=float(density), dtype=compute)
        values = np.asarray(density, dtype=self.compute_dtype)
        if values.shape != tuple(self.grid.shape):
            raise ValueError(f"density of component {name} must be a number or an array of the grid's shape {tuple(self.grid.shape)}, got {values.shape}")
        if not (values > 0).all():
            raise ValueError(f"prepare_fields: the density of component {name} must be positive everywhere (the scheme divides by it), "
                             f"its minimum is {values.min()}")
        rho = self.grid.create_field(cardinality=1, dtype=compute)
        rho.assign(values[None])
        return rho

    def prepare_fields(self, density=(1.0, 1.0), initializer=None):
        """f^s_0 = feq(density[s], u = 0); ``density``: a pair, each a positive number or an array of the grid's shape.  ``initializer``
        (bc_mask, fA_0, fB_0) -> (fA_0, fB_0) replaces it."""
        keep = lambda bc_mask, f_0: f_0
        fa_0, fa_1, bc_mask, missing_mask = super().prepare_fields(initializer=keep)
        fb_0 = self.grid.create_field(cardinality=self.velocity_set.q, dtype=self.precision_policy.store_precision)
        fb_1 = self.grid.create_field(cardinality=self.velocity_set.q, dtype=self.precision_policy.store_precision)
        if initializer is not None:
            fa_0, fb_0 = initializer(bc_mask, fa_0, fb_0)
        else:
            if not isinstance(density, (tuple, list)) or len(density) != 2:
                raise ValueError("density takes a pair (rho_A, rho_B)")
            fields = [self._density_field(rho, name) for rho, name in zip(density, "AB")]
            fa_0 = initialize_eq(fa_0, self.grid, self.velocity_set, self.precision_policy, self.compute_backend, rho=fields[0])
            fb_0 = initialize_eq(fb_0, self.grid, self.velocity_set, self.precision_policy, self.compute_backend, rho=fields[1])
            self._ctx.sync()
            for rho in fields:
                rho.free()
        return fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega, timestep):
        omega_a, omega_b = self._omegas(omega)
        self._multicomponent_native().step(fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega_a, omega_b, timestep)
        return fa_0, fa_1, fb_0, fb_1

    def run(self, fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """``n_steps`` x (step, swap) in native code, nothing waits for the device; returns (fA, fA_other, fB, fB_other) with the
        fields that hold the result first."""
        omega_a, omega_b = self._omegas(omega)
        in_1 = self._multicomponent_native().run(fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega_a, omega_b, first_timestep, n_steps)
        return (fa_1, fa_0, fb_1, fb_0) if in_1 else (fa_0, fa_1, fb_0, fb_1)

    def run_timed(self, *args, **kwargs):
        raise NotImplementedError("MulticomponentStepper has no run_timed: bracket run() with ctx.sync() and a wall clock")

    def _output(self, cardinality):
        return self.grid.create_field(cardinality=cardinality, dtype=self.precision_policy.compute_precision)

    def densities(self, fa, fb, bc_mask, missing_mask):
        """rho_A, rho_B of the post-streaming state as the force reads them (the wall pair at fullway and solid cells)"""
        rho_a, rho_b = self._output(1), self._output(1)
        self._multicomponent_native().densities(fa, fb, bc_mask, missing_mask, rho_a, rho_b)
        return rho_a, rho_b

    def interaction_force(self, fa, fb, bc_mask, missing_mask):
        """F^A, F^B of the post-streaming state, without ``force_vector``, the lattice's d components each"""
        force_a, force_b = self._output(self.velocity_set.d), self._output(self.velocity_set.d)
        self._multicomponent_native().force(fa, fb, bc_mask, missing_mask, force_a, force_b)
        return force_a, force_b

    def macroscopic(self, fa, fb, bc_mask, missing_mask):
        """rho_A, rho_B and the barycentric velocity of the post-streaming state of the stored fields"""
        rho_a, rho_b, u = self._output(1), self._output(1), self._output(self.velocity_set.d)
        self._multicomponent_native().macroscopic(fa, fb, bc_mask, missing_mask, rho_a, rho_b, u)
        return rho_a, rho_b, u
