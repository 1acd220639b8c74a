"""NumPy restatement of the coupled fluid + scalar step of ScalarTransportStepper (csrc/scalar_kernels.hpp, scalar_step_kernel.hpp).

TEST INFRASTRUCTURE ONLY.  The fluid half is built from the oracle's operators (oracle/xlb_numpy.py: stream, apply_bc, macroscopic,
equilibrium, the collisions, assemble_auxiliary_data) in the order of its ``step``; the scalar half is stated here.  The reference has
no scalar transport (it only names PhysicsType.ADE), so the scheme is pinned by the physics checks of tests/test_scalar_ref.py.

The step, in the compute dtype T (sums sequential in direction order, no FMA):
  1. S = pull stream of F0 + the fluid's streaming BCs
  2. R[j] = roll(G0[j], c_j); at cells with a bc id, for every scalar direction j whose FLUID missing bit is set:
     Dirichlet  R[j] = -G0[opp j] + (T(2) T(w_j)) T(value);  adiabatic (the default)  R[j] = G0[opp j];
     at do-nothing cells R[:] = G0[:]
  3. phi = sum_j R[j]
  4. rho, u = moments of S
  5. the fluid collides; with a force or buoyancy through the exact-difference path with force + buoyancy (phi - reference) per cell
  6. geq_j = (T(w_j) phi) (T(1) + T(1 / cs^2) (c_j . u));  G1 = R - T(omega_s) (R - geq)
  7. at fullway cells G1[j] = R[opp j]
  8. both fields are stored in the store dtype
"""

import numpy as np

from oracle import xlb_numpy as orc

ADIABATIC, DIRICHLET, DO_NOTHING = "adiabatic", "dirichlet", "do_nothing"


class ScalarLattice:
    """Rest direction + the fluid lattice's main directions in ascending order: D2Q5 / D3Q7."""

    def __init__(self, lat):
        self.lat = lat
        self.dirs = np.concatenate([[lat.center], np.sort(lat.main)]).astype(np.int64)  # fluid direction of scalar direction j
        self.q = len(self.dirs)
        assert self.q == 2 * lat.d + 1
        self.c = lat.c[:, self.dirs]  # (d, q)
        fluid_opp = lat.opp[self.dirs]
        self.opp = np.array([int(np.nonzero(self.dirs == o)[0][0]) for o in fluid_opp])
        w0, wj, self.inv_cs2 = (1.0 / 4.0, 1.0 / 8.0, 4.0) if lat.d == 3 else (1.0 / 3.0, 1.0 / 6.0, 3.0)
        self.w = np.array([w0] + [wj] * (self.q - 1))
        self.cs2 = 1.0 / self.inv_cs2

    def diffusivity(self, omega_s):
        return self.cs2 * (1.0 / omega_s - 0.5)


class Rule:
    def __init__(self, kind, bc_id, value=0.0):
        self.kind, self.id, self.value = kind, int(bc_id), float(value)


def equilibrium_g(phi, u, sl, T):
    """geq_j = (w_j phi) (1 + c_j.u / cs^2); every scalar direction has at most one non-zero component"""
    phi = np.asarray(phi, dtype=T)
    u = np.asarray(u, dtype=T)
    geq = np.empty((sl.q,) + phi.shape, dtype=T)
    for j in range(sl.q):
        cu = np.zeros(phi.shape, dtype=T)
        for a in range(sl.lat.d):
            if sl.c[a, j] == 1:
                cu = u[a]
            elif sl.c[a, j] == -1:
                cu = -u[a]
        geq[j] = (T(sl.w[j]) * phi) * (T(1) + T(sl.inv_cs2) * cu)
    return geq


def scalar_sum(g):
    phi = g[0].copy()
    for j in range(1, g.shape[0]):
        phi = phi + g[j]
    return phi


def scalar_stream(G0, bc_mask, missing_mask, rules, sl):
    """step 2; returns R and, per rule, the number of (cell, direction) links it acted on"""
    T = G0.dtype.type
    d = sl.lat.d
    R = np.empty_like(G0)
    for j in range(sl.q):
        R[j] = np.roll(G0[j], tuple(int(s) for s in sl.c[:, j]), axis=tuple(range(d)))
    by_id = {r.id: r for r in rules}
    ids = bc_mask[0]
    acted = {}
    mm = missing_mask.astype(bool)
    for bc_id in np.unique(ids[ids != 0]):
        rule = by_id.get(int(bc_id), Rule(ADIABATIC, bc_id))
        cells = ids == bc_id
        if rule.kind == DO_NOTHING:
            R = np.where(cells[None], G0, R)
            acted[int(bc_id)] = int(cells.sum())
            continue
        n = 0
        for j in range(1, sl.q):
            cond = cells & mm[sl.dirs[j]]
            n += int(cond.sum())
            if rule.kind == DIRICHLET:
                R[j] = np.where(cond, -G0[sl.opp[j]] + (T(2) * T(sl.w[j])) * T(rule.value), R[j])
            else:
                R[j] = np.where(cond, G0[sl.opp[j]], R[j])
        acted[int(bc_id)] = n
    return R, acted


def scalar_collide(R, phi, u, omega_s, sl, fullway):
    """steps 6 and 7; fullway: boolean cell mask or None"""
    T = R.dtype.type
    geq = equilibrium_g(phi, u, sl, T)
    G1 = R - T(omega_s) * (R - geq)
    if fullway is not None and fullway.any():
        G1 = np.where(fullway[None], R[sl.opp], G1)
    return G1


def _fullway_cells(bc_mask, bcs):
    cells = np.zeros(bc_mask.shape[1:], dtype=bool)
    for bc in bcs:
        if bc.kind == orc.KIND_FULLWAY_BB:
            cells |= bc_mask[0] == bc.id
    return cells


def init_g(phi0, f_0, lat, policy="FP32FP32"):
    """g_0 = geq(phi0, u(f_0)) in the store dtype"""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    sl = ScalarLattice(lat)
    _, u = orc.macroscopic(f_0.astype(T), lat)
    phi = np.broadcast_to(np.asarray(phi0, dtype=T), f_0.shape[1:]).astype(T)
    return equilibrium_g(phi, u, sl, T).astype(S)


def moment(g, policy="FP32FP32"):
    return scalar_sum(g.astype(orc.compute_dtype(policy)))[None]


def step(f_0, g_0, bc_mask, missing_mask, bcs, rules, omega, omega_s, lat, policy="FP32FP32", collision="BGK", force_vector=None, buoyancy=None,
         reference=0.0, acted=None):
    """One coupled step -> (f_1, g_1) in the store dtype."""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    sl = ScalarLattice(lat)
    F0, G0 = f_0.astype(T), g_0.astype(T)
    post_stream = orc.stream(F0, lat)
    for bc in bcs:
        if bc.step == orc.STEP_STREAMING:
            post_stream = orc.apply_bc(bc, F0, post_stream, bc_mask, missing_mask, lat, policy)
    R, n_acted = scalar_stream(G0, bc_mask, missing_mask, rules, sl)
    if acted is not None:
        acted.update(n_acted)
    phi = scalar_sum(R)
    rho, u = orc.macroscopic(post_stream, lat)
    feq = orc.equilibrium(rho, u, lat, T)
    if collision == "BGK":
        post_coll = orc.bgk(post_stream, feq, omega)
    elif collision == "KBC":
        post_coll = orc.kbc(post_stream, feq, omega, lat)
    elif collision == "SmagorinskyLESBGK":
        post_coll = orc.smagorinsky_les_bgk(post_stream, feq, omega, lat)
    else:
        raise ValueError(collision)
    if force_vector is not None or buoyancy is not None:
        fv = np.zeros(lat.d) if force_vector is None else np.asarray(force_vector, dtype=np.float64)
        bv = np.zeros(lat.d) if buoyancy is None else np.asarray(buoyancy, dtype=np.float64)
        dphi = phi - T(reference)
        du = np.stack([T(fv[a]) + T(bv[a]) * dphi for a in range(lat.d)])
        rho2, u2 = orc.macroscopic(post_coll, lat)
        post_coll = post_coll + (orc.equilibrium(rho2, u2 + du, lat, T) - feq)  # exact_difference_force with a per-cell force
    for bc in bcs:
        post_coll = orc.assemble_auxiliary_data(bc, post_stream, post_coll, bc_mask, missing_mask, lat)
        if bc.step == orc.STEP_COLLISION:
            post_coll = orc.apply_bc(bc, post_stream, post_coll, bc_mask, missing_mask, lat, policy)
    G1 = scalar_collide(R, phi, u, omega_s, sl, _fullway_cells(bc_mask, bcs))
    return post_coll.astype(S), G1.astype(S)


def run(f_0, g_0, bc_mask, missing_mask, bcs, rules, omega, omega_s, lat, n_steps, **kw):
    f, g = f_0, g_0
    for _ in range(n_steps):
        f, g = step(f, g, bc_mask, missing_mask, bcs, rules, omega, omega_s, lat, **kw)
    return f, g


def scalar_step(g_0, u, bc_mask, missing_mask, rules, omega_s, lat, policy="FP32FP32", fullway=None):
    """The scalar half alone in a GIVEN velocity field u (d, *shape): what the coupled step does to g when the flow is u."""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    sl = ScalarLattice(lat)
    R, _ = scalar_stream(g_0.astype(T), bc_mask, missing_mask, rules, sl)
    return scalar_collide(R, scalar_sum(R), np.asarray(u, dtype=T), omega_s, sl, fullway).astype(S)
