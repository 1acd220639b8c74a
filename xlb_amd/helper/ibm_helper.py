"""Set-up helpers of the immersed-boundary stepper (reference xlb/helper/ibm_helper.py:11-24 and :118-205).

Mesh subdivision (the reference's ``prepare_immersed_boundary`` goes through trimesh) is not part of this backend: bring markers
that are about one cell apart.

``RigidMotion`` and ``IBMBody`` describe bodies with prescribed motion for ``IBMStepper.set_bodies`` (the reference's
examples/ibm/wind_turbine_ibm.py:160-199 turns its rotor with a kernel of its own; here the host evaluates poses and the stepper's
native code applies them).  ``RigidDynamics`` describes a free body, which the stepper's native code integrates from its loads."""

from types import SimpleNamespace

import numpy as np

from .nse_fields import create_nse_fields


def create_ibm_fields(grid_shape, velocity_set=None, precision_policy=None):
    """-> (grid, f_0, f_1, missing_mask, bc_mask) for an IBMStepper (ibm_helper.py:11-24)."""
    return create_nse_fields(grid_shape=grid_shape, velocity_set=velocity_set, precision_policy=precision_policy)


def calculate_voronoi_areas(vertices, faces):
    """Area that each vertex of a triangle mesh stands for: every face's area is split among its corners by the normalised cotangent
    weights of ibm_helper.py:166-183 (corner 0 gets A (cot_beta + cot_gamma) / 2 with the three cotangents scaled to sum to one, and
    so on), so the areas add up to the mesh's.  ``vertices`` (n, 3), ``faces`` (m, 3) vertex indices -> (n,) float32."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(faces, dtype=np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("vertices must be (n, 3) and faces (m, 3)")
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)
    a2 = ((p1 - p2) ** 2).sum(axis=1)
    b2 = ((p0 - p2) ** 2).sum(axis=1)
    c2 = ((p0 - p1) ** 2).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cot = np.stack([b2 + c2 - a2, a2 + c2 - b2, a2 + b2 - c2]) / (4.0 * area)  # alpha, beta, gamma: the angles at p0, p1, p2
        total = cot.sum(axis=0)
        cot = np.where(total > 0, cot / total, cot)
    cot = np.where(area > 0, cot, 0.0)  # (degenerate faces carry no area)
    out = np.zeros(v.shape[0])
    np.add.at(out, t[:, 0], area * cot[1] / 2.0 + area * cot[2] / 2.0)
    np.add.at(out, t[:, 1], area * cot[0] / 2.0 + area * cot[2] / 2.0)
    np.add.at(out, t[:, 2], area * cot[0] / 2.0 + area * cot[1] / 2.0)
    return out.astype(np.float32)


def icosphere(subdivisions=2):
    """Unit icosphere: (vertices (n, 3) float64, faces (m, 3)); n = 10 * 4^subdivisions + 2."""
    g = (1.0 + 5.0**0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts), np.array(faces, dtype=np.int64)


class RigidMotion:
    """Constant rotation about ``axis`` through ``centre`` by ``rate`` radians per step, plus a constant translation of the centre by
    ``velocity`` per step; ``phase`` is the angle at timestep 0.

    ``at(timestep)`` -> ``(R (3, 3), c (3,), w (3,), v (3,))`` in float64: the rotation by the TOTAL angle phase + rate * timestep
    (Rodrigues' formula on that one angle, never a product of per-step rotations, so it cannot drift), the centre
    centre + velocity * timestep, the angular velocity rate * axis / |axis| and the velocity of the centre.  Any object with such an
    ``at`` is a motion as far as ``IBMStepper`` is concerned (an oscillating cylinder, a pitching foil, a spin-up ramp, ...)."""

    def __init__(self, centre, axis, rate, velocity=(0.0, 0.0, 0.0), phase=0.0):
        self.centre = np.array(centre, dtype=np.float64).reshape(3)
        axis = np.array(axis, dtype=np.float64).reshape(3)
        norm = float(np.sqrt((axis * axis).sum()))
        if not norm > 0.0:
            raise ValueError("RigidMotion: the axis must not be zero")
        self.axis = axis / norm
        self.rate = float(rate)
        self.velocity = np.array(velocity, dtype=np.float64).reshape(3)
        self.phase = float(phase)

    def at(self, timestep):
        angle = self.phase + self.rate * float(timestep)
        x, y, z = self.axis
        K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
        R = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
        return R, self.centre + self.velocity * float(timestep), self.rate * self.axis, self.velocity.copy()


def _finite(name, value, shape=None):
    a = np.array(value, dtype=np.float64)
    if shape is not None:
        try:
            a = np.broadcast_to(a, shape).copy()
        except ValueError:
            raise ValueError(f"RigidDynamics: {name} must have shape {shape}") from None
    if not np.isfinite(a).all():
        raise ValueError(f"RigidDynamics: {name} is not finite")
    return a


class RigidDynamics:
    """A FREE rigid body: its pose is not prescribed but integrated on the device, once per step, from the force and the torque the
    coupling has just found for it (``IBMBody(markers, dynamics=RigidDynamics(...))``).

    ``mass``              the effective mass the integrator divides by (> 0)
    ``inertia``           the effective inertia tensor in the BODY frame, 3 x 3 symmetric positive definite; a scalar: that multiple
                          of the identity
    ``centre, velocity``  position and velocity of the centre at timestep 0 (lattice units)
    ``orientation``       3 x 3 rotation at timestep 0 (default: the identity)
    ``angular_velocity``  at timestep 0, a world-frame vector in radians per step
    ``force, torque``     constant external loads in the world frame (the buoyancy-corrected weight goes here)
    ``spring``            (anchor, stiffness, damping): a linear tether that adds -stiffness (c - anchor) - damping v per axis;
                          stiffness and damping are 3-vectors or scalars
    ``translate``         which world axes the centre may move along
    ``rotate``            "free" (3-D rotation), ("axis", a) (about the fixed world direction a through the centre: a free-spinning
                          rotor) or "locked"
    ``virtual_mass``      m_v >= 0 and
    ``virtual_inertia``   I_v >= 0 (added as I_v E to the body-frame inertia): the virtual-mass stabilisation of Schwarz, Kempe and
                          Froehlich (J. Comput. Phys. 281 (2015) 591).  The term is added to both sides of the equation of motion, on
                          the right with the previous step's acceleration: a = (F + m_v a_prev) / (mass + m_v), and T + I_v alpha_prev
                          for the torque.  A steady state is unchanged; transients are slowed

    The scheme is explicit with dt = 1 (csrc/ibm_dynamics_kernels.hpp states it to the operation): symplectic Euler for the centre,
    v' = v + F / mass, c' = c + v', and for the rotation L' = L + T, w* = R Ib^-1 R^T L', q' = normalise(cay(w*) q) with the Cayley
    map in place of the exponential.  Explicit coupling of this kind is unstable for bodies about as light as the fluid unless a
    virtual mass is set; see ``sphere``.  Contact forces with planes and between bodies are switched on with
    ``IBMStepper.set_contact`` for bodies that carry an ``IBMBody(..., contact_radius=r)``; there are no lubrication, tangential or
    frictional forces, and a body must stay two cells inside the box (no periodic wrap), which wall planes can enforce."""

    ROTATE_LOCKED, ROTATE_AXIS, ROTATE_FREE = 0, 1, 2

    def __init__(self, mass, inertia, centre, velocity=(0.0, 0.0, 0.0), orientation=None, angular_velocity=(0.0, 0.0, 0.0), force=(0.0, 0.0, 0.0),
                 torque=(0.0, 0.0, 0.0), spring=None, translate=(True, True, True), rotate="free", virtual_mass=0.0, virtual_inertia=0.0):
        self.mass = float(_finite("mass", mass, ()))
        if not self.mass > 0.0:
            raise ValueError("RigidDynamics: mass must be positive")
        inertia = _finite("inertia", inertia)
        if inertia.ndim == 0:
            inertia = float(inertia) * np.eye(3)
        if inertia.shape != (3, 3) or not np.array_equal(inertia, inertia.T) or not (np.linalg.eigvalsh(inertia) > 0.0).all():
            raise ValueError("RigidDynamics: inertia must be a positive scalar or a 3 x 3 symmetric positive definite tensor")
        self.inertia = inertia
        self.virtual_mass = float(_finite("virtual_mass", virtual_mass, ()))
        self.virtual_inertia = float(_finite("virtual_inertia", virtual_inertia, ()))
        if self.virtual_mass < 0.0:
            raise ValueError("RigidDynamics: virtual_mass must not be negative")
        if self.virtual_inertia < 0.0:
            raise ValueError("RigidDynamics: virtual_inertia must not be negative")
        self.centre = _finite("centre", centre, (3,))
        self.velocity = _finite("velocity", velocity, (3,))
        self.orientation = np.eye(3) if orientation is None else _finite("orientation", orientation, (3, 3))
        if np.abs(self.orientation.T @ self.orientation - np.eye(3)).max() > 1e-12 or np.linalg.det(self.orientation) < 0.0:
            raise ValueError("RigidDynamics: orientation must be a rotation matrix")
        self.angular_velocity = _finite("angular_velocity", angular_velocity, (3,))
        self.force = _finite("force", force, (3,))
        self.torque = _finite("torque", torque, (3,))
        if spring is None:
            self.anchor, self.stiffness, self.damping = np.zeros(3), np.zeros(3), np.zeros(3)
        else:
            try:
                anchor, stiffness, damping = spring
            except (TypeError, ValueError):
                raise ValueError("RigidDynamics: spring must be (anchor, stiffness, damping)") from None
            self.anchor = _finite("spring", anchor, (3,))
            self.stiffness = _finite("spring", stiffness, (3,))
            self.damping = _finite("spring", damping, (3,))
        translate = np.array(translate, dtype=bool)
        if translate.shape != (3,):
            raise ValueError("RigidDynamics: translate must be three booleans")
        self.translate = translate
        self.axis = np.zeros(3)
        if isinstance(rotate, str) and rotate in ("free", "locked"):
            self.rotate = self.ROTATE_FREE if rotate == "free" else self.ROTATE_LOCKED
        elif isinstance(rotate, (tuple, list)) and len(rotate) == 2 and rotate[0] == "axis":
            axis = _finite("axis", rotate[1], (3,))
            norm = float(np.sqrt((axis * axis).sum()))
            if not norm > 0.0:
                raise ValueError("RigidDynamics: the axis must not be zero")
            self.axis = axis / norm
            self.rotate = self.ROTATE_AXIS
        else:
            raise ValueError('RigidDynamics: rotate must be "free", "locked" or ("axis", a)')

    @classmethod
    def sphere(cls, radius, density, centre, gravity=(0.0, 0.0, 0.0), virtual_mass_coefficient=0.0, **kw):
        """A homogeneous sphere of ``density`` (the fluid's is 1) under ``gravity``, with Uhlmann's (J. Comput. Phys. 209 (2005) 448)
        effective quantities: the fluid inside the marker surface is forced too and moves with the body, which leaves
        mass = (density - 1) V, inertia = (density - 1) 2/5 V r^2 and force = (density - 1) V g for the integrator.

        density <= 1.2 is refused: with the effective mass tending to zero the explicit scheme is unstable below about that ratio
        (Uhlmann reports the limit); lighter bodies need a virtual mass: ``virtual_mass_coefficient`` = C_v > 0 sets
        virtual_mass = C_v V and virtual_inertia = C_v 2/5 V r^2, and then any density above 1 is taken.  In the NumPy restatement
        of the coupled loop (a 24^3 box, radius 5.3, four sweeps; profiles/ibm_virtual_mass.md) C_v = 4 holds density 2.5 (3 does not),
        C_v = 6 and 8 hold densities 1.15 (4 does not) and 1.05; the rotational counterpart was not measured."""
        radius, density = float(radius), float(density)
        if not radius > 0.0 or not np.isfinite(radius):
            raise ValueError("RigidDynamics.sphere: radius must be positive")
        coefficient = float(_finite("virtual_mass_coefficient", virtual_mass_coefficient, ()))
        if coefficient < 0.0:
            raise ValueError("RigidDynamics.sphere: virtual_mass_coefficient must not be negative")
        if coefficient > 0.0:
            if not density > 1.0:
                raise ValueError("RigidDynamics.sphere: density must exceed 1 (the effective mass (density - 1) V must be positive)")
        elif not density > 1.2:
            raise ValueError("RigidDynamics.sphere: density must exceed 1.2 (the explicit coupling is unstable for lighter bodies)")
        volume = 4.0 / 3.0 * np.pi * radius**3
        excess = (density - 1.0) * volume
        g = _finite("gravity", gravity, (3,))
        if coefficient > 0.0:
            kw.update(virtual_mass=coefficient * volume, virtual_inertia=coefficient * 0.4 * volume * radius * radius)
        return cls(mass=excess, inertia=excess * 0.4 * radius * radius, centre=centre, force=excess * g, **kw)

    uhlmann = sphere

    @staticmethod
    def _quaternion(R):
        """Unit quaternion (w, x, y, z) of a rotation matrix (the branch with the largest pivot)."""
        t = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]])
        k = int(np.argmax(t))
        r = np.sqrt(1.0 + t[k])
        if k == 0:
            q = np.array([r * r, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        elif k == 1:
            q = np.array([R[2, 1] - R[1, 2], r * r, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
        elif k == 2:
            q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], r * r, R[1, 2] + R[2, 1]])
        else:
            q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], r * r])
        q = q / (2.0 * r)
        return q / np.sqrt((q * q).sum())

    def native(self):
        """-> (rotation mode, 32 parameters, 16 doubles of initial state) as xlbhip_ibm_set_dynamics takes them: the host passes
        1 / mass, Ib^-1, 1 / I_a with I_a = a^T R0 Ib R0^T a, and L(0) = R0 Ib R0^T w0 (axis mode: the rate a . w0).  With a virtual
        mass or inertia, mass + m_v and Ib + I_v E take the places of mass and Ib in these; m_v and I_v themselves travel separately
        (``virtual()``)."""
        R0 = self.orientation
        inertia = self.inertia + self.virtual_inertia * np.eye(3) if self.virtual_inertia > 0.0 else self.inertia
        mass = self.mass + self.virtual_mass if self.virtual_mass > 0.0 else self.mass
        world = R0 @ inertia @ R0.T
        params = np.zeros(32)
        params[0] = 1.0 / mass
        params[1:4] = self.translate.astype(np.float64)
        params[4:7], params[7:10] = self.force, self.torque
        params[10:13], params[13:16], params[16:19] = self.anchor, self.stiffness, self.damping
        params[19:28] = np.linalg.inv(inertia).reshape(9)
        state = np.zeros(16)
        state[0:3], state[3:6] = self.centre, self.velocity
        state[6:10] = self._quaternion(R0)
        if self.rotate == self.ROTATE_AXIS:
            params[28:31] = self.axis
            params[31] = 1.0 / float(self.axis @ world @ self.axis)
            state[10] = float(self.axis @ self.angular_velocity)
        elif self.rotate == self.ROTATE_FREE:
            state[10:13] = world @ self.angular_velocity
        return self.rotate, params, state

    def virtual(self):
        """-> (m_v, I_v) as xlbhip_ibm_set_virtual_mass takes them."""
        return self.virtual_mass, self.virtual_inertia


class IBMBody:
    """A contiguous range of an IBMStepper's markers that moves as one rigid body.

    ``markers``   slice(a, b) into the marker arrays (step 1)
    ``motion``    a RigidMotion, any object with its ``at(timestep)``, or None
    ``dynamics``  a RigidDynamics: the body is free, moved by the loads on it; not together with ``motion``.  With neither the body
                  is at rest (its loads are still summed)
    ``centre0``   the point the uploaded vertices refer to: marker k sits at c(t) + R(t) (X0_k - centre0).  Default: motion.at(0)[1],
                  dynamics.centre, or the mean of the body's markers for a body at rest (there it is the point the torque is taken
                  about).
    ``contact_radius``  r > 0: the body takes part in the contact model of ``IBMStepper.set_contact`` as a sphere of that radius
                  about its centre — a free body is pushed, a prescribed body or one at rest is an obstacle.  None: it does not."""

    def __init__(self, markers, motion=None, centre0=None, dynamics=None, contact_radius=None):
        if not isinstance(markers, slice):
            raise TypeError("IBMBody: markers must be a slice of the marker arrays")
        if motion is not None and dynamics is not None:
            raise TypeError("IBMBody: motion and dynamics are mutually exclusive")
        if motion is not None and not callable(getattr(motion, "at", None)):
            raise TypeError("IBMBody: motion must be None or have an at(timestep) method")
        if dynamics is not None and not isinstance(dynamics, RigidDynamics):
            raise TypeError("IBMBody: dynamics must be None or a RigidDynamics")
        self.markers = markers
        self.motion = motion
        self.dynamics = dynamics
        self.centre0 = None if centre0 is None else np.array(centre0, dtype=np.float64).reshape(3)
        if contact_radius is not None:
            contact_radius = float(contact_radius)
            if not (np.isfinite(contact_radius) and contact_radius > 0.0):
                raise ValueError("IBMBody: contact_radius must be positive and finite, or None")
        self.contact_radius = contact_radius


def declare_bodies(bodies, n_markers, uploaded_positions, max_bodies=64):
    """What ``IBMStepper.set_bodies`` hands to the native object for a list of IBMBody over ``n_markers`` markers; needs no device.
    ``uploaded_positions()`` -> the (n_markers, 3) positions uploaded last, asked for only when a resting body with markers has
    no ``centre0`` (it gets the mean of its markers).  Raises ValueError naming the body for a range that is out of bounds or
    overlaps another, and for more than ``max_bodies`` bodies.

    -> ``ranges`` [(a, b)], ``kinds`` (0 at rest, 1 prescribed, 2 dynamic), ``centre0`` (n, 3), ``radius`` (n,) contact radii with
    0 for none, ``virtual`` (n, 2) m_v | I_v, and — None unless some body is dynamic — ``rotate`` (n,), ``params`` (n, 32),
    ``state`` (n, 16) as xlbhip_ibm_set_dynamics takes them."""
    if len(bodies) > max_bodies:
        raise ValueError(f"set_bodies: {len(bodies)} bodies, at most {max_bodies} are supported")
    n = n_markers
    ranges = []
    for i, body in enumerate(bodies):
        if not isinstance(body, IBMBody):
            raise TypeError(f"set_bodies: body {i} is not an IBMBody")
        sl = body.markers
        a, b = (0 if sl.start is None else sl.start), (n if sl.stop is None else sl.stop)
        if sl.step not in (None, 1):
            raise ValueError(f"set_bodies: body {i}: the markers must be a contiguous range (slice step {sl.step})")
        if not 0 <= a <= b <= n:
            raise ValueError(f"set_bodies: body {i}: markers {a}:{b} are out of bounds for {n} markers")
        for j, (c, d) in enumerate(ranges):
            if a < d and c < b:
                raise ValueError(f"set_bodies: bodies {j} and {i} overlap (markers {c}:{d} and {a}:{b})")
        ranges.append((a, b))
    centre0 = np.zeros((len(bodies), 3))
    uploaded = None
    for i, (body, (a, b)) in enumerate(zip(bodies, ranges)):
        if body.centre0 is not None:
            centre0[i] = body.centre0
        elif body.motion is not None:
            centre0[i] = np.asarray(body.motion.at(0)[1], dtype=np.float64)
        elif body.dynamics is not None:
            centre0[i] = body.dynamics.centre
        elif b > a:
            uploaded = uploaded_positions() if uploaded is None else uploaded
            centre0[i] = uploaded[a:b].astype(np.float64).mean(axis=0)
    kinds = [2 if body.dynamics is not None else int(body.motion is not None) for body in bodies]
    out = SimpleNamespace(ranges=ranges, kinds=kinds, centre0=centre0, rotate=None, params=None, state=None)
    out.radius = np.array([0.0 if body.contact_radius is None else body.contact_radius for body in bodies], dtype=np.float64)
    out.virtual = np.array([(0.0, 0.0) if body.dynamics is None else body.dynamics.virtual() for body in bodies], dtype=np.float64).reshape(-1, 2)
    if 2 in kinds:
        out.rotate, out.params, out.state = np.zeros(len(bodies), np.int32), np.zeros((len(bodies), 32)), np.zeros((len(bodies), 16))
        for i, body in enumerate(bodies):
            if body.dynamics is not None:
                out.rotate[i], out.params[i], out.state[i] = body.dynamics.native()
    return out
