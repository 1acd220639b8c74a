"""NumPy restatement of the free-body integrator WITH virtual mass and contact (k_ibm_integrate_contact of
xlb_amd/csrc/ibm_dynamics_kernels.hpp), test infrastructure only.  It extends tests/_ibm_dynamics_ref.py, which it changes nothing
in, and keeps its rule: every line is one fp64 operation on np.float64 scalars in the order written.

On top of (rotate, P, S) of tests/_ibm_dynamics_ref.py a body carries
    virt = (m_v, I_v)          the virtual mass and inertia; P[0], P[19:28], P[31] already hold 1 / (mass + m_v), (Ib + I_v E)^-1,
                               1 / (I_a + I_v), as RigidDynamics.native() passes them
    prev = a_prev | alpha_prev 6 doubles, zero at the start
and the contact model is ``Contact``: radii (0 = the body takes no part), range, stiffness, wall stiffness, planes lo / hi.
"""

import numpy as np

from _ibm_dynamics_ref import AXIS, D, FREE, LOCKED, angular_velocity, cayley_step, pose, quat_matrix  # noqa: F401

DYNAMIC = 2


class Contact:
    def __init__(self, radius, range, stiffness, wall_stiffness=None, lo=None, hi=None):
        self.radius = np.asarray(radius, D)
        self.range, self.stiffness = D(range), D(stiffness)
        self.wall_stiffness = self.stiffness if wall_stiffness is None else D(wall_stiffness)
        self.lo = np.full(3, -np.inf) if lo is None else np.asarray(lo, D)
        self.hi = np.full(3, np.inf) if hi is None else np.asarray(hi, D)


def contact_force(i, centres, model):
    """The force on body i from the planes (axis by axis, lo before hi) and then from the bodies j in ascending order; centres (n, 3)
    are the c of the step's poses."""
    C = np.asarray(centres, D)
    r, zeta = model.radius, model.range
    Fc = [D(0.0)] * 3
    with np.errstate(all="ignore"):
        for a in range(3):
            gap = (C[i, a] - model.lo[a]) - r[i]
            if gap < zeta:
                p = zeta - gap
                Fc[a] = Fc[a] + model.wall_stiffness * (p * p)
            gap = (model.hi[a] - C[i, a]) - r[i]
            if gap < zeta:
                p = zeta - gap
                Fc[a] = Fc[a] + (-(model.wall_stiffness * (p * p)))
        for j in range(len(C)):
            if j == i or not r[j] > 0.0:
                continue
            e = [C[i, a] - C[j, a] for a in range(3)]
            d = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            gap = d - (r[i] + r[j])
            if gap < zeta and d > 0.0:
                p = zeta - gap
                s = model.stiffness * (p * p)
                for a in range(3):
                    Fc[a] = Fc[a] + (s * e[a]) / d
    return np.array(Fc, D)


def integrate(rotate, P, S, loads, virt=(0.0, 0.0), prev=None, Fc=None):
    """State of t -> state of t + 1.  Fc: the contact force (3,) of a body that takes part, else None.
    -> (new state (16,), new prev (6,), ok); when a component is not finite the old state AND the old prev come back."""
    P, S, H = np.asarray(P, D), np.asarray(S, D), np.asarray(loads, D)
    A = np.zeros(6, D) if prev is None else np.asarray(prev, D)
    mv, iv = D(virt[0]), D(virt[1])
    new, nprev = S.copy(), np.zeros(6, D)
    with np.errstate(all="ignore"):
        for a in range(3):
            c, v = S[a], S[3 + a]
            F = ((H[a] + P[4 + a]) + (-(P[13 + a] * (c - P[10 + a])))) + (-(P[16 + a] * v))
            if Fc is not None:
                F = F + Fc[a]
            acc = (F + mv * A[a]) * P[0] if mv > 0.0 else F * P[0]
            ta = P[1 + a] * acc
            vn = v + ta
            new[3 + a] = vn
            new[a] = c + vn
            nprev[a] = ta
        q = S[6:10]
        T = [H[3 + a] + P[7 + a] for a in range(3)]
        if iv > 0.0:
            T = [T[a] + iv * A[3 + a] for a in range(3)]
        if rotate != LOCKED:
            if rotate == FREE:
                for a in range(3):
                    new[10 + a] = S[10 + a] + T[a]
            else:
                new[10] = S[10] + ((P[28] * T[0] + P[29] * T[1]) + P[30] * T[2]) * P[31]
            R = quat_matrix(q)
            th = angular_velocity(rotate, R, new[10:13], P)
            new[6:10] = cayley_step(th, q)
            w0 = angular_velocity(rotate, R, S[10:13], P)
            for a in range(3):
                nprev[3 + a] = th[a] - w0[a]
    if not (np.isfinite(new[:13]).all() and np.isfinite(nprev).all()):
        return S.copy(), A.copy(), False
    return new, nprev, True


def step_bodies(kind, rotate, P, S, loads, virt, prev, centres, model):
    """One launch of k_ibm_integrate_contact on all bodies: kind (n,), rotate (n,), P (n, 32), S (n, 16), loads (n, 6), virt (n, 2),
    prev (n, 6), centres (n, 3) of the step's poses, model a Contact or None.  -> (S', prev', contact (n, 3), ok (n,))."""
    n = len(kind)
    S2, prev2, contact, ok = np.array(S, D), np.array(prev, D), np.zeros((n, 3), D), np.ones(n, bool)
    for b in range(n):
        if kind[b] != DYNAMIC:
            continue
        Fc = None
        if model is not None and model.radius[b] > 0.0:
            Fc = contact_force(b, centres, model)
            contact[b] = Fc
        S2[b], prev2[b], ok[b] = integrate(int(rotate[b]), P[b], S[b], loads[b], virt[b], prev[b], Fc)
    return S2, prev2, contact, ok


def replay(kind, rotate, P, S0, loads_history, virt, model=None, staged=None):
    """Feed recorded loads (n_steps, n, 6) to all bodies.  staged (n_steps + 1, n, 18): the pose rows of the bodies that are not
    dynamic (their c is what the contact reads).  -> (poses (n_steps + 1, n, 18), states, prevs, contacts (n_steps, n, 3))."""
    kind = np.asarray(kind)
    n = len(kind)
    S, prev = np.array(S0, D), np.zeros((n, 6), D)

    def rows(t):
        out = np.zeros((n, 18), D)
        for b in range(n):
            out[b] = pose(int(rotate[b]), P[b], S[b]) if kind[b] == DYNAMIC else staged[t][b]
        return out

    poses, states, prevs, contacts = [rows(0)], [S.copy()], [prev.copy()], []
    for t, H in enumerate(np.asarray(loads_history, D)):
        S, prev, contact, ok = step_bodies(kind, rotate, P, S, H, virt, prev, poses[-1][:, 9:12], model)
        assert ok.all()
        poses.append(rows(t + 1))
        states.append(S.copy())
        prevs.append(prev.copy())
        contacts.append(contact)
    return np.array(poses), np.array(states), np.array(prevs), np.array(contacts)


def coupled_run(dynamics, X0, areas, f0, lat, policy, collision, steps, omega, ibm, model=None):
    """tests/_ibm_dynamics_ref.coupled_run for ONE free body that owns all markers, with its virtual mass and, with ``model`` (one
    radius), the planes' contact force.  -> dict(f, forces, poses (steps + 1, 18), loads (steps, 6), contact (steps, 3), ...)."""
    import _ibm_motion_ref as mref
    import _ibm_ref as ref

    rotate, P, S = dynamics.native()
    virt, prev = dynamics.virtual(), np.zeros(6, D)
    o_bm, o_mm = np.zeros((1,) + f0.shape[1:], np.uint8), np.zeros((lat.q,) + f0.shape[1:], bool)
    out = {"f": f0}
    poses, loads, contacts = [], [], []
    for _ in range(steps):
        row = pose(rotate, P, S)
        X, V = mref.move(X0, dynamics.centre, row[:9].reshape(3, 3), row[9:12], row[12:15], row[15:18])
        out = ref.step(out["f"], X, areas, V, o_bm, o_mm, [], omega, lat, policy, collision, **ibm)
        H = mref.loads_tree(out["forces"], areas, X, row[9:12])
        Fc = contact_force(0, row[None, 9:12], model) if model is not None and model.radius[0] > 0.0 else None
        S, prev, ok = integrate(rotate, P, S, H, virt, prev, Fc)
        assert ok
        poses.append(row)
        loads.append(H)
        contacts.append(np.zeros(3) if Fc is None else Fc)
    poses.append(pose(rotate, P, S))
    out.update(poses=np.array(poses), loads=np.array(loads), contact=np.array(contacts), positions=X, velocities=V)
    return out
