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

Bodies that move.  A rigid body with PRESCRIBED motion is declared once and moved on the device (the reference's
examples/ibm/wind_turbine_ibm.py:160-199 does the same with a kernel of its own, ``rotate_rotor``):

    stepper.set_bodies([IBMBody(markers=slice(0, 600), motion=RigidMotion(centre, axis, rate)), IBMBody(markers=slice(600, 900))])
    f_0, f_1, history = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n, record_loads=True)    # (n, n_bodies, 6)

The call with timestep t places marker k of body b at X_k(t) = c_b(t) + R_b(t) (X0_k - c0_b) with velocity
U_k(t) = v_b(t) + w_b(t) x (X_k(t) - c_b(t)), where X0 are the vertices last uploaded (``markers.update(vertices=...)`` replaces
them), c0_b is the body's ``centre0`` and (R, c, w, v) = ``motion.at(t)``.  The ``velocities`` uploaded for the markers of a moving
body are IGNORED.  A body with ``motion=None`` is at rest; markers in no body stay as uploaded.  ``body_loads()`` is the force and
the torque on every body in the last call.

Free bodies.  ``IBMBody(markers=..., dynamics=RigidDynamics(mass, inertia, centre, ...))`` declares a body whose motion is NOT
prescribed: after the loads of every step one tiny kernel advances its centre, velocity, orientation and angular momentum from
them (explicit, dt = 1; helper/ibm_helper.py and csrc/ibm_dynamics_kernels.hpp state the scheme), and the next step's move reads
the new pose — a settling particle, a sphere on an elastic mount, a rotor the flow spins up.  The state lives on the device: a
``run`` with free bodies and no prescribed mover is ONE native call with no pose staging, and nothing in it waits for the device or
reads from it.  Free, prescribed and resting bodies mix in one ``set_bodies``; a new ``set_bodies`` resets the state to the declared
initial values.  ``body_poses()`` is the pose (R | c | w | v, 18 doubles per body) the next call will use;
``run(..., record_poses=True)`` also returns the poses every step used, row for row with ``record_loads``.  A body whose new state
is not finite stops where it is and ``body_poses()`` raises, naming it.  The integration is explicit: ``set_bodies`` warns
(RuntimeWarning) when a free body's mass plus virtual mass is below ibm_max_iterations x the sum of its markers' areas, the added
mass the coupling can load it with, beyond which the scheme diverges unless the sweeps end early.

Light bodies and contact.  ``RigidDynamics(..., virtual_mass=, virtual_inertia=)`` or ``RigidDynamics.sphere(...,
virtual_mass_coefficient=C_v)`` adds the virtual-mass term of Schwarz, Kempe and Froehlich (2015) to the integrator, which is what a
body about as dense as the fluid needs.  ``set_contact(range, stiffness, wall_stiffness, box)`` switches on a central repulsive
force between the bodies that carry an ``IBMBody(..., contact_radius=r)`` and from the planes of ``box``; ``body_contact_forces()``
reads the last step's.  Both are evaluated inside the integrator's launch: a light sphere that settles onto a floor is still one
native ``run``.  A stepper that uses neither enqueues exactly the launches it did before.  Measured (profiles/ibm_virtual_mass.md):
the NumPy restatement of the coupled loop, translation only, on a 24^3 box — C_v = 4 holds a sphere of density 2.5 and C_v = 8 one
of density 1.15 with all four sweeps, where no virtual mass diverges; the device replays the restatement bit for bit.  NOT measured:
the rotational counterpart in a coupled run, and any settling curve against an experiment.

Not covered: lubrication, tangential or frictional contact; a body crossing a periodic face (the coupling does not wrap: keep bodies
two cells inside the box, e.g. with the planes of ``set_contact``); deformable bodies.

The host evaluates the poses (18 doubles per step and body) and stages them ahead of the steps, as it does for time-dependent
walls: ``run`` works in chunks of at most POSE_CHUNK_STEPS = 256 steps and at most 1 MiB of poses (113 steps with 64 bodies); the
poses of the next chunk are evaluated while the device runs the current one, and nothing inside a chunk waits for the device.

3-D lattices, fp32 / fp64 storage, one rank."""

import warnings

import numpy as np

from ... import _lib
from ...helper.ibm_helper import IBMBody, RigidDynamics, RigidMotion, declare_bodies  # noqa: F401  (re-exported: they are this stepper's vocabulary)
from ...compute_backend import ComputeBackend
from ..operator import Operator
from .nse_stepper import IncompressibleNavierStokesStepper, refuse_regularized, refuse_unsupported


class IBMMarkers:
    """The markers of an IBMStepper on the device (there is one set per stepper)."""

    def __init__(self, stepper):
        self._stepper = stepper
        self._areas = None  # host copy of the areas last uploaded (set_bodies checks the mass of free bodies against them)

    def __len__(self):
        return self._stepper._ibm_native().n

    def update(self, vertices=None, areas=None, velocities=None):
        """Replace any of the three arrays (same number of markers), or all three with a new number of markers (not while bodies are
        declared).  ``vertices`` are the reference positions of the bodies that move; their ``velocities`` are ignored."""
        given = [a for a in (vertices, areas, velocities) if a is not None]
        n = len(given[0]) if given else len(self)
        self._stepper._ibm_native().set_markers(n, vertices, areas, velocities)
        if areas is not None:
            self._areas = np.array(areas, dtype=np.float32).reshape(-1)
        return self

    def positions(self):
        """The positions the device holds now — after the last call's move — as (n, 3) float32.  Synchronous."""
        return self._stepper._ibm_native().download_markers(velocities=False)[0]

    def velocities(self):
        """The velocities the device holds now, (n, 3) float32.  Synchronous."""
        return self._stepper._ibm_native().download_markers(positions=False)[1]


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
        refuse_regularized("IBMStepper", collision_type)
        # the pairing of reference-style calls is off: every call runs its step at once
        super().__init__(grid, boundary_conditions, collision_type=collision_type, backend_config={"lazy_pairs": False})
        if self.velocity_set.d != 3:
            raise NotImplementedError("IBMStepper: 2-D grids are not supported (the coupling kernels are written for D3Q19 / D3Q27)")
        refuse_unsupported("IBMStepper", self.precision_policy, grid)
        self.use_scoped_timer = bool(use_scoped_timer)  # (accepted for the reference's signature; timing is run_timed's job here)
        self.ibm_max_iterations = int(ibm_max_iterations)
        self.ibm_tolerance = float(ibm_tolerance)
        self.ibm_relaxation = float(ibm_relaxation)
        if not 0 <= self.ibm_max_iterations <= 64:
            raise ValueError("ibm_max_iterations must be 0 .. 64")
        if self.ibm_tolerance < 0:
            raise ValueError("ibm_tolerance must not be negative")
        self._ibm = None
        self._bodies = []
        self._any_prescribed = False  # some body with markers follows a prescribed motion: its poses are staged
        self._any_dynamic = False
        self._contact = None  # (range, stiffness, wall_stiffness, lo, hi) of set_contact
        self._next_timestep = 0
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

    # -- rigid bodies -----------------------------------------------------------------------------------------------
    MAX_BODIES = 64
    POSE_CHUNK_STEPS = 256  # steps whose poses run() evaluates and stages at once, further capped by _lib.IBM.POSE_BYTES

    def set_bodies(self, bodies):
        """Declare the rigid bodies: a list of IBMBody over disjoint contiguous ranges of the markers uploaded before (``[]``: none,
        today's plain stepper; markers a device has moved stay where they are).  Raises ValueError naming the body for a range that
        is out of bounds or overlaps another, and for more than 64 bodies."""
        bodies = list(bodies)
        ibm = self._ibm_native()
        d = declare_bodies(bodies, ibm.n, self._markers.positions, self.MAX_BODIES)
        ibm.set_bodies([a for a, _ in d.ranges], [b - a for a, b in d.ranges], d.kinds, d.centre0)
        self._any_dynamic = 2 in d.kinds
        if self._any_dynamic:
            self._warn_light_bodies(bodies, d.ranges)
            ibm.set_dynamics(d.rotate, d.params, d.state)
            if (d.virtual > 0.0).any():
                ibm.set_virtual_mass(d.virtual[:, 0], d.virtual[:, 1])
        self._bodies = bodies
        self._body_centre0 = d.centre0
        self._body_radius = d.radius
        self._next_timestep = 0  # (body_poses: a new declaration starts over, for prescribed bodies as for free ones)
        self._any_prescribed = any(body.motion is not None and b > a for body, (a, b) in zip(bodies, d.ranges))
        self._apply_contact()

    def set_contact(self, range, stiffness, wall_stiffness=None, box=None):
        """Switch on the contact model for the bodies declared with an ``IBMBody(..., contact_radius=r)``, now and in every later
        ``set_bodies``: a central repulsive soft-sphere force of the Glowinski / Wan-Turek kind, evaluated on the device inside the
        integrator's launch from the centres of the step's poses.

        ``range``           zeta >= 0: the force acts while the gap between two surfaces is below it
        ``stiffness``       k >= 0: body i gets k (zeta - gap)^2 (c_i - c_j) / |c_i - c_j| from every body j with a radius, with
                            gap = |c_i - c_j| - (r_i + r_j).  Prescribed bodies and bodies at rest are obstacles; only free bodies
                            are pushed
        ``wall_stiffness``  k_w >= 0 (default: ``stiffness``): k_w (zeta - gap)^2 along the inward normal of a plane of ``box``,
                            gap = (distance of the centre from the plane) - r_i
        ``box``             (lo, hi), 3 values each: the planes x_a = lo_a and x_a = hi_a; -inf / +inf switch a plane off.  None: no
                            planes.  Planes two cells plus zeta inside the grid keep the markers' supports inside it

        A body at rest on a plane under a weight W sits where k_w (zeta - gap)^2 = W: choose k_w zeta^2 well above W.  The force is
        explicit, so k (k_w) must stay well below (mass + virtual mass) / dt^2 = the mass in lattice units.  It enters the
        integrator only: ``body_loads()`` stays hydrodynamic.  Raises ValueError naming the argument that is negative or not finite,
        or the axis with lo >= hi."""
        def number(name, value):
            value = float(value)
            if not (np.isfinite(value) and value >= 0.0):
                raise ValueError(f"set_contact: {name} must be finite and not negative")
            return value

        zeta, k = number("range", range), number("stiffness", stiffness)
        kw = k if wall_stiffness is None else number("wall_stiffness", wall_stiffness)
        lo = hi = None
        if box is not None:
            try:
                lo, hi = (np.array(x, dtype=np.float64).reshape(3) for x in box)
            except (TypeError, ValueError):
                raise ValueError("set_contact: box must be (lo, hi) with 3 values each") from None
            for a in (0, 1, 2):
                if not lo[a] < hi[a]:
                    raise ValueError(f"set_contact: box: lo >= hi along axis {a} ({lo[a]} and {hi[a]})")
        self._contact = (zeta, k, kw, lo, hi)
        self._apply_contact()

    def _apply_contact(self):
        if self._contact is None or not self._any_dynamic:
            return
        self._ibm_native().set_contact(self._body_radius, *self._contact)

    def body_contact_forces(self):
        """(n_bodies, 3) float64: the contact force on every body in the LAST call, read from the device now (zero for bodies that
        are not free or carry no ``contact_radius``, and while no ``set_contact`` is in force)."""
        if not self._bodies:
            return np.zeros((0, 3))
        return self._ibm_native().contact_forces()

    def _warn_light_bodies(self, bodies, ranges):
        """The marker force is the velocity deficit added up over the sweeps that ran, so a body that starts to move drags an added
        mass of up to ibm_max_iterations x (sum of its markers' areas) along; the explicit integrator diverges when that exceeds
        the body's mass plus its virtual mass.  Say so when the body is declared, not when its state has stopped being finite."""
        areas = self._markers._areas
        if areas is None:
            return
        for i, (body, (a, b)) in enumerate(zip(bodies, ranges)):
            dyn = body.dynamics
            if dyn is None or not dyn.translate.any():
                continue
            added = self.ibm_max_iterations * float(areas[a:b].astype(np.float64).sum())
            if dyn.mass + dyn.virtual_mass < added:
                what = f"mass {dyn.mass:.4g}" if dyn.virtual_mass == 0.0 else f"mass + virtual mass {dyn.mass + dyn.virtual_mass:.4g}"
                warnings.warn(f"set_bodies: body {i}: {what} is below ibm_max_iterations x sum of marker areas = {added:.4g}, the added mass the "
                              "coupling can load it with; the explicit integration of this body is unstable unless the sweeps end early "
                              "(heavier body, a virtual mass, fewer sweeps, or a smaller ibm_relaxation)", RuntimeWarning, stacklevel=3)

    def _poses(self, t_first, n):
        """(n, n_bodies, 18) float64: R (row-major) | c | w | v of every body at t_first .. t_first + n - 1 (the rest pose for a
        dynamic body, whose row the device ignores)."""
        out = np.zeros((n, len(self._bodies), 18))
        for i, body in enumerate(self._bodies):
            if body.motion is None:
                out[:, i, 0] = out[:, i, 4] = out[:, i, 8] = 1.0
                out[:, i, 9:12] = self._body_centre0[i]
                continue
            for k in range(n):
                R, c, w, v = body.motion.at(int(t_first) + k)
                row = out[k, i]
                row[0:9] = np.asarray(R, dtype=np.float64).reshape(9)
                row[9:12], row[12:15], row[15:18] = c, w, v
        return out

    def _pose_chunk(self):
        return max(1, min(self.POSE_CHUNK_STEPS, _lib.IBM.POSE_BYTES // (18 * 8 * len(self._bodies))))

    def body_loads(self):
        """(n_bodies, 6) float64 of the LAST call, read from the device now: columns 0-2 the force on the body, -sum_k A_k F_k,
        columns 3-5 the torque on it about the body's centre c_b at that step, -sum_k A_k (X_k - c_b) x F_k."""
        return self._ibm_native().loads()

    def body_poses(self):
        """(n_bodies, 18) float64, R (row-major) | c | w | v of every body as the NEXT call will use it, read from the device now: the
        integrated state of a free body, ``motion.at`` of the timestep after the last call's for a prescribed one, the rest pose
        otherwise.  Raises RuntimeError naming the free bodies that met a state that was not finite (they have stood still since)."""
        if not self._bodies:
            return np.zeros((0, 18))
        poses, status = self._ibm_native().body_poses()
        if status:
            bad = [i for i in range(len(self._bodies)) if status >> i & 1]
            raise RuntimeError(f"body_poses: the state of bodies {bad} stopped being finite (loads too large for the explicit integrator?)")
        if self._any_prescribed:
            staged = self._poses(self._next_timestep, 1)[0]
            for i, body in enumerate(self._bodies):
                if body.motion is not None:
                    poses[i] = staged[i]
        return poses

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f_0, f_1, vertices, areas, velocities, bc_mask, missing_mask, omega, timestep):
        self._set_markers(vertices, areas, velocities)
        self._stage(timestep, 1)
        if self._any_prescribed:
            self._ibm_native().stage_poses(timestep, self._poses(timestep, 1))
        self._ibm_native().step(f_0, f_1, bc_mask, missing_mask, omega, timestep)
        self._next_timestep = int(timestep) + 1
        return f_0, f_1, self.s_lagr_forces

    def run(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0, record_loads=False, record_poses=False):
        """``n_steps`` x (move the bodies, step with the coupling, loads, integrate the free bodies, swap) in native code; returns
        (f_current, f_other), with ``record_loads`` also the loads of every step, (n_steps, n_bodies, 6), and with ``record_poses``
        also the poses every step's move and loads read, (n_steps, n_bodies, 18) — in that order; both are written on the device and
        read once after the run."""
        ibm = self._ibm_native()
        n_steps, first_timestep = int(n_steps), int(first_timestep)
        record = bool(record_loads) and len(self._bodies) > 0 and n_steps > 0
        if record:
            ibm.record_loads(n_steps)
        record_p = bool(record_poses) and len(self._bodies) > 0 and n_steps > 0
        if record_p:
            ibm.record_poses(n_steps)
        cur, oth = f_0, f_1
        try:
            if self._time_dependent_bcs():
                for k in range(n_steps):
                    self._stage(first_timestep + k, 1)
                    if self._any_prescribed:
                        ibm.stage_poses(first_timestep + k, self._poses(first_timestep + k, 1))
                    ibm.step(cur, oth, bc_mask, missing_mask, omega, first_timestep + k)
                    cur, oth = oth, cur
            elif self._any_prescribed:
                chunk, done = self._pose_chunk(), 0
                poses = self._poses(first_timestep, min(chunk, n_steps))
                while done < n_steps:
                    m = len(poses)
                    ibm.stage_poses(first_timestep + done, poses)
                    if ibm.run(cur, oth, bc_mask, missing_mask, omega, first_timestep + done, m):
                        cur, oth = oth, cur
                    done += m
                    if done < n_steps:  # (the device is busy with the chunk just enqueued)
                        poses = self._poses(first_timestep + done, min(chunk, n_steps - done))
            elif ibm.run(f_0, f_1, bc_mask, missing_mask, omega, first_timestep, n_steps):
                cur, oth = f_1, f_0
            self._next_timestep = first_timestep + n_steps
            out = (cur, oth)
            if record_loads:
                out += (ibm.loads_history(n_steps) if record else np.zeros((n_steps, len(self._bodies), 6)),)
            if record_poses:
                out += (ibm.poses_history(n_steps) if record_p else np.zeros((n_steps, len(self._bodies), 18)),)
        finally:  # also when a step was refused: a recording left on would add launches to every later run
            if record:
                ibm.record_loads(0)
            if record_p:
                ibm.record_poses(0)
        return out

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
