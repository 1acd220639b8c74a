"""NumPy restatement of the two-component Shan-Chen step of MulticomponentStepper (csrc/multicomponent_kernels.hpp,
multicomponent_step_kernel.hpp).

TEST INFRASTRUCTURE ONLY.  The front half of each component is tests/_multiphase_ref.py's (the oracle's stream, apply_bc and macroscopic
in the order of its ``step``); the common velocity, the two forces and the collision are stated here.  The reference has no
multicomponent flow, so the scheme is pinned by the physics checks of tests/test_multicomponent_ref.py.

The step, in the compute dtype T (sums sequential in direction order, no FMA), s in {A, B}:
  1. S^s = pull stream of f^s + the streaming BCs (halfway bounce-back at rest); rho_s, u_s = moments of S^s
  2. psi_s = rho_s; at wall cells (fullway bounce-back cells, cells of bc id 255) psi_s = rho_w,s of the cell's id
  3. for i = 1 .. q-1 ascending: psi_s,i = rho_w,s of the cell's OWN id where the cell has an id and its missing bit opp(i) is set, else
     psi_s[x + c_i] (periodic);  t = T(w_i) psi_s,i;  S^s_a = S^s_a + t where c_ai = 1, S^s_a - t where c_ai = -1
  4. F^A_a = (-rho_A) ((T(G_AA) S^A_a) + (T(G_AB) S^B_a)),  F^B_a = (-rho_B) ((T(G_AB) S^A_a) + (T(G_BB) S^B_a)),  zero at wall cells
  5. wa = T(omega_A) rho_A, wb = T(omega_B) rho_B;  u'_a = ((wa u_A,a) + (wb u_B,a)) / (wa + wb)
  6. feq = feq(rho_s, u');  f^s = (S^s - T(omega_s) (S^s - feq)) + (feq(rho_s, u' + (T(force_a) + F^s_a / rho_s)) - feq)
  7. fullway cells take S^s[opp] instead; the result is stored in the store dtype
Physical velocity of the outputs: (((rho_A u_A) + (rho_B u_B)) + (F^A + F^B) / T(2)) / (rho_A + rho_B).
"""

import numpy as np

from oracle import xlb_numpy as orc

import _multiphase_ref as mp

BC_SOLID = mp.BC_SOLID
CS2 = 1.0 / 3.0
no_walls = mp.no_walls
wall_cells = mp.wall_cells


class Mixture:
    def __init__(self, G_AB, G_AA=0.0, G_BB=0.0):
        self.G_AB, self.G_AA, self.G_BB = float(G_AB), float(G_AA), float(G_BB)


def pressure(mix, rho_a, rho_b):
    """bulk equation of state, in fp64"""
    a, b = np.asarray(rho_a, dtype=np.float64), np.asarray(rho_b, dtype=np.float64)
    return CS2 * (a + b) + CS2 * (0.5 * mix.G_AA * a * a + mix.G_AB * a * b + 0.5 * mix.G_BB * b * b)


def wall_tables(wall_density, T):
    """two [256] tables of rho_w by bc id in T; wall_density: {bc id: (rho_w of A, rho_w of B)}, every other id 0"""
    ta, tb = np.zeros(256, dtype=T), np.zeros(256, dtype=T)
    for bc_id, (a, b) in (wall_density or {}).items():
        ta[int(bc_id)], tb[int(bc_id)] = T(a), T(b)
    return ta, tb


def stencil_sums(psi, own_wall, bc_mask, missing_mask, lat):
    """step 3 for one component -> list of d arrays"""
    T = psi.dtype.type
    ids = bc_mask[0]
    mm = missing_mask.astype(bool)
    axes = tuple(range(lat.d))
    S = [np.zeros(psi.shape, dtype=T) for _ in range(lat.d)]
    for i in range(1, lat.q):
        neighbour = np.roll(psi, tuple(-int(s) for s in lat.c[:, i]), axis=axes)
        psi_i = np.where((ids != 0) & mm[lat.opp[i]], own_wall, neighbour)
        t = T(lat.w[i]) * psi_i
        for a in range(lat.d):
            if lat.c[a, i] == 1:
                S[a] = S[a] + t
            elif lat.c[a, i] == -1:
                S[a] = S[a] - t
    return S


def step(fa_0, fb_0, bc_mask, missing_mask, bcs, omega, lat, mix, wall_density=None, policy="FP32FP32", force_vector=None, parts=None):
    """One step -> (f^A_1, f^B_1) in the store dtype.  omega: (omega_A, omega_B) or one number.  parts: a dict that receives rho_a, rho_b
    (moments), psi_a, psi_b (what the force reads), ua, ub (bare), uc (u'), force_a, force_b and u_phys."""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    omega_a, omega_b = (omega, omega) if np.ndim(omega) == 0 else omega
    ta, tb = wall_tables(wall_density, T)
    ids = bc_mask[0]
    walls = wall_cells(bc_mask, bcs)
    post_a, rho_a, ua = mp.front(fa_0, bc_mask, missing_mask, bcs, lat, policy)
    post_b, rho_b, ub = mp.front(fb_0, bc_mask, missing_mask, bcs, lat, policy)
    psi_a = np.where(walls, ta[ids], rho_a[0])
    psi_b = np.where(walls, tb[ids], rho_b[0])
    Sa = stencil_sums(psi_a, ta[ids], bc_mask, missing_mask, lat)
    Sb = stencil_sums(psi_b, tb[ids], bc_mask, missing_mask, lat)
    gaa, gab, gbb = T(mix.G_AA), T(mix.G_AB), T(mix.G_BB)
    na, nb = -rho_a[0], -rho_b[0]
    Fa = np.stack([np.where(walls, T(0), na * ((gaa * Sa[a]) + (gab * Sb[a]))) for a in range(lat.d)])
    Fb = np.stack([np.where(walls, T(0), nb * ((gab * Sa[a]) + (gbb * Sb[a]))) for a in range(lat.d)])
    fv = np.zeros(lat.d) if force_vector is None else np.asarray(force_vector, dtype=np.float64)
    with np.errstate(all="ignore"):
        wa, wb = T(omega_a) * rho_a[0], T(omega_b) * rho_b[0]
        den = wa + wb
        uc = np.stack([((wa * ua[a]) + (wb * ub[a])) / den for a in range(lat.d)])
        out = []
        for post, rho, F, om in ((post_a, rho_a, Fa, omega_a), (post_b, rho_b, Fb, omega_b)):
            us = np.stack([uc[a] + (T(fv[a]) + F[a] / rho[0]) for a in range(lat.d)])
            feq = orc.equilibrium(rho, uc, lat, T)
            post_coll = orc.bgk(post, feq, om) + (orc.equilibrium(rho, us, lat, T) - feq)
            for bc in bcs:
                if bc.step == orc.STEP_COLLISION:
                    post_coll = orc.apply_bc(bc, post, post_coll, bc_mask, missing_mask, lat, policy)
            out.append(post_coll.astype(S))
        if parts is not None:
            u_phys = np.stack([(((rho_a[0] * ua[a]) + (rho_b[0] * ub[a])) + (Fa[a] + Fb[a]) / T(2)) / (rho_a[0] + rho_b[0]) for a in range(lat.d)])
            parts.update(rho_a=rho_a, rho_b=rho_b, psi_a=psi_a[None], psi_b=psi_b[None], ua=ua, ub=ub, uc=uc, force_a=Fa, force_b=Fb, u_phys=u_phys)
    return out[0], out[1]


def run(fa, fb, bc_mask, missing_mask, bcs, omega, lat, mix, n_steps, **kw):
    for _ in range(n_steps):
        fa, fb = step(fa, fb, bc_mask, missing_mask, bcs, omega, lat, mix, **kw)
    return fa, fb


def outputs(fa, fb, bc_mask, missing_mask, bcs, lat, mix, wall_density=None, policy="FP32FP32"):
    """the parts of the post-streaming state of the stored fields"""
    parts = {}
    step(fa, fb, bc_mask, missing_mask, bcs, 1.0, lat, mix, wall_density, policy, parts=parts)
    return parts


init_at_rest = mp.init_at_rest
