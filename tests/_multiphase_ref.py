"""NumPy restatement of the Shan-Chen step of MultiphaseStepper (csrc/multiphase_kernels.hpp, multiphase_step_kernel.hpp).

TEST INFRASTRUCTURE ONLY.  The fluid half is built from the oracle's operators (oracle/xlb_numpy.py: stream, apply_bc, macroscopic,
equilibrium, bgk) in the order of its ``step``; the pseudopotentials and the interaction force are stated here.  The reference has no
multiphase flow, so the scheme is pinned by the physics checks of tests/test_multiphase_ref.py.

The step, in the compute dtype T (sums sequential in direction order, no FMA):
  1. S = pull stream of F0 + the streaming BCs (halfway bounce-back); rho, u = moments of S
  2. psi = Psi(rho); at wall cells (fullway bounce-back cells, cells of bc id 255) psi = Psi(rho_w) of the cell's id
  3. for i = 1 .. q-1 ascending: psi_i = Psi(rho_w) of the cell's OWN id where the cell has an id and its missing bit opp(i) is set,
     else psi[x + c_i] (periodic);  t = T(w_i) psi_i;  S_a = S_a + t where c_ai = 1, S_a - t where c_ai = -1
  4. F_a = (T(-G) psi) S_a, zero at wall cells
  5. BGK, then the exact-difference shift with the per-cell acceleration T(force_a) + F_a / rho
  6. fullway cells take S[opp] instead; the result is stored in the store dtype
Physical velocity of the outputs: u + F / (T(2) rho).
"""

import numpy as np

from oracle import xlb_numpy as orc

BC_SOLID = 255
CS2 = 1.0 / 3.0


class Exponential:
    """psi = rho0 (1 - exp(-rho / rho0))"""

    def __init__(self, G, rho0=1.0):
        self.G, self.rho0 = float(G), float(rho0)

    def psi(self, rho):
        rho = np.asarray(rho)
        T = rho.dtype.type
        return T(self.rho0) * (T(1) - np.exp(-(rho / T(self.rho0))))


class Density:
    """psi = rho"""

    def __init__(self, G):
        self.G = float(G)

    def psi(self, rho):
        return np.asarray(rho).copy()


class CarnahanStarling:
    """psi = sqrt(2 (p - cs2 rho) / (G cs2)), G = -1, p = rho R T (1 + eta + eta^2 - eta^3) / (1 - eta)^3 - a rho^2, eta = b rho / 4"""

    G = -1.0

    def __init__(self, T, a=1.0, b=4.0, R=1.0):
        self.T, self.a, self.b, self.R = float(T), float(a), float(b), float(R)

    @staticmethod
    def critical_temperature(a=1.0, b=4.0, R=1.0):
        return 0.3773 * a / (b * R)

    def eos(self, rho):
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


def pressure(model, rho):
    """bulk equation of state cs2 rho + (G cs2 / 2) psi^2, in fp64"""
    rho = np.asarray(rho, dtype=np.float64)
    return CS2 * rho + 0.5 * model.G * CS2 * model.psi(rho) ** 2


def wall_table(model, wall_density, T):
    """[256] Psi(rho_w) by bc id in T; wall_density: {bc id: rho_w}, every other id 0"""
    table = np.zeros(256, dtype=T)
    with np.errstate(all="ignore"):
        for bc_id, rho_w in (wall_density or {}).items():
            table[int(bc_id)] = model.psi(np.array(rho_w, dtype=T))
    return table


def wall_cells(bc_mask, bcs):
    cells = bc_mask[0] == BC_SOLID
    for bc in bcs:
        if bc.kind == orc.KIND_FULLWAY_BB:
            cells = cells | (bc_mask[0] == bc.id)
    return cells


def front(f_0, bc_mask, missing_mask, bcs, lat, policy):
    """step 1: (post-streaming populations, rho, u) in the compute dtype"""
    T = orc.compute_dtype(policy)
    F0 = f_0.astype(T)
    post_stream = orc.stream(F0, lat)
    for bc in bcs:
        if bc.step == orc.STEP_STREAMING:
            post_stream = orc.apply_bc(bc, F0, post_stream, bc_mask, missing_mask, lat, policy)
    rho, u = orc.macroscopic(post_stream, lat)
    return post_stream, rho, u


def psi_field(rho, bc_mask, bcs, model, table):
    """step 2 -> (1, *shape)"""
    with np.errstate(all="ignore"):
        psi = model.psi(rho[0])
    return np.where(wall_cells(bc_mask, bcs), table[bc_mask[0]], psi)[None]


def interaction_force(psi, bc_mask, missing_mask, bcs, model, table, lat):
    """steps 3 and 4 -> (d, *shape)"""
    T = psi.dtype.type
    p = psi[0]
    ids = bc_mask[0]
    mm = missing_mask.astype(bool)
    own_wall = table[ids]
    axes = tuple(range(lat.d))
    S = [np.zeros(p.shape, dtype=T) for _ in range(lat.d)]
    for i in range(1, lat.q):
        neighbour = np.roll(p, tuple(-int(s) for s in lat.c[:, i]), axis=axes)
        psi_i = np.where((ids != 0) & mm[lat.opp[i]], own_wall, neighbour)
        t = T(lat.w[i]) * psi_i
        for a in range(lat.d):
            if lat.c[a, i] == 1:
                S[a] = S[a] + t
            elif lat.c[a, i] == -1:
                S[a] = S[a] - t
    gp = T(-model.G) * p
    zero = wall_cells(bc_mask, bcs)
    return np.stack([np.where(zero, T(0), gp * S[a]) for a in range(lat.d)])


def step(f_0, bc_mask, missing_mask, bcs, omega, lat, model, wall_density=None, policy="FP32FP32", force_vector=None, psi=None, parts=None):
    """One step -> f_1 in the store dtype.  psi: a (1, *shape) field to use instead of step 2 (the device's, for the exponential form
    whose exp is not NumPy's).  parts: a dict that receives rho, u (bare), psi, force and u_phys."""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    table = wall_table(model, wall_density, T)
    post_stream, rho, u = front(f_0, bc_mask, missing_mask, bcs, lat, policy)
    if psi is None:
        psi = psi_field(rho, bc_mask, bcs, model, table)
    psi = np.asarray(psi, dtype=T)
    F = interaction_force(psi, bc_mask, missing_mask, bcs, model, table, lat)
    fv = np.zeros(lat.d) if force_vector is None else np.asarray(force_vector, dtype=np.float64)
    with np.errstate(all="ignore"):
        du = np.stack([T(fv[a]) + F[a] / rho[0] for a in range(lat.d)])
        feq = orc.equilibrium(rho, u, lat, T)
        post_coll = orc.bgk(post_stream, feq, omega)
        rho2, u2 = orc.macroscopic(post_coll, lat)
        post_coll = post_coll + (orc.equilibrium(rho2, u2 + du, lat, T) - feq)  # exact_difference_force with a per-cell force
        for bc in bcs:
            if bc.step == orc.STEP_COLLISION:
                post_coll = orc.apply_bc(bc, post_stream, post_coll, bc_mask, missing_mask, lat, policy)
        if parts is not None:
            parts.update(rho=rho, u=u, psi=psi, force=F, u_phys=np.stack([u[a] + F[a] / (T(2) * rho[0]) for a in range(lat.d)]))
    return post_coll.astype(S)


def run(f_0, bc_mask, missing_mask, bcs, omega, lat, model, n_steps, **kw):
    f = f_0
    for _ in range(n_steps):
        f = step(f, bc_mask, missing_mask, bcs, omega, lat, model, **kw)
    return f


def outputs(f, bc_mask, missing_mask, bcs, lat, model, wall_density=None, policy="FP32FP32", psi=None):
    """rho, u_phys, psi, force of the post-streaming state of the stored field f"""
    parts = {}
    step(f, bc_mask, missing_mask, bcs, 1.0, lat, model, wall_density, policy, psi=psi, parts=parts)
    return parts


def init_at_rest(density, lat, policy="FP32FP32"):
    """f = feq(density, 0) in the store dtype"""
    T = orc.compute_dtype(policy)
    rho = np.asarray(density, dtype=T)[None]
    return orc.equilibrium(rho, np.zeros((lat.d,) + rho.shape[1:], T), lat, T).astype(orc.store_dtype(policy))


def no_walls(shape, lat):
    return np.zeros((1,) + tuple(shape), np.uint8), np.zeros((lat.q,) + tuple(shape), bool)
