"""Set-up helpers of the immersed-boundary stepper (reference xlb/helper/ibm_helper.py:11-24 and :118-205).

Mesh subdivision (the reference's ``prepare_immersed_boundary`` goes through trimesh) is not part of this backend: bring markers
that are about one cell apart.

``RigidMotion`` and ``IBMBody`` describe bodies with prescribed motion for ``IBMStepper.set_bodies`` (the reference's
examples/ibm/wind_turbine_ibm.py:160-199 turns its rotor with a kernel of its own; here the host evaluates poses and the stepper's
native code applies them)."""

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


class IBMBody:
    """A contiguous range of an IBMStepper's markers that moves as one rigid body.

    ``markers``  slice(a, b) into the marker arrays (step 1)
    ``motion``   a RigidMotion, any object with its ``at(timestep)``, or None for a body at rest (whose loads are still summed)
    ``centre0``  the point the uploaded vertices refer to: marker k sits at c(t) + R(t) (X0_k - centre0).  Default: motion.at(0)[1],
                 or the mean of the body's markers for a body at rest (there it is the point the torque is taken about)."""

    def __init__(self, markers, motion=None, centre0=None):
        if not isinstance(markers, slice):
            raise TypeError("IBMBody: markers must be a slice of the marker arrays")
        if motion is not None and not callable(getattr(motion, "at", None)):
            raise TypeError("IBMBody: motion must be None or have an at(timestep) method")
        self.markers = markers
        self.motion = motion
        self.centre0 = None if centre0 is None else np.array(centre0, dtype=np.float64).reshape(3)
