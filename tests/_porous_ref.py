"""NumPy restatement of the porous BGK step and of its discrete adjoint (csrc/porous_kernels.hpp, porous_step_kernel.hpp).

TEST INFRASTRUCTURE ONLY.  Built on the oracle's operators (oracle/xlb_numpy.py) and on the adjoint restatement (tests/_adjoint_ref.py:
post_stream, stream_transpose) as that one is built on the oracle.  The forward step is the oracle's BGK step with the equilibrium taken
at the damped velocity; tests/test_porous_ref.py pins it to the oracle at alpha == 0 and pins the transposed rules to it by finite
differences.

alpha: one value per cell, shape (1,) + grid, the compute dtype.  In the compute dtype T, every sum sequential and no FMA:

  forward   1. fs = pull stream of f_n + the streaming BCs (f*); rho, u of fs as the oracle computes them
            2. kappa = 1 - alpha;  ut_d = kappa u_d;  feq = the oracle's equilibrium at (rho, ut)
            3. f_out = fs - omega (fs - feq);  fullway cells: f_out_l = fs_[opp l];  stored in the store dtype
  adjoint   1. as forward 1 and 2, usqr = 1.5 sum_d ut_d ut_d
            2. per direction k = 0 .. q-1 (cu_k = 3 (c_k . ut), e_k = (1 + cu_k (1 + 0.5 cu_k)) - usqr, s_k = 3 (1 + cu_k)):
                   A    += lam_k (w_k e_k)
                   B_d  += lam_k ((rho w_k) g_dk),  d ascending,  g_dk = s_k - 3 ut_d | (-s_k) - 3 ut_d | -(3 ut_d)  for c_dk = 1 | -1 | 0
                   term += lam_k (feq_k - fs_k)
               (the first term starts each sum)
            3. Br_d = (kappa B_d) / rho;  mu_j = (1 - omega) lam_j + omega (A + sum_d Br_d (c_dj - u_d)),  the sum started at A,
               d ascending, c_dj - u_d = 1 - u_d | -1 - u_d | -u_d  (u, not ut)
            4. galpha = -(omega s),  s = sum_d B_d u_d,  d ascending, the first product starts the sum
            5. fullway cells: mu_j = lam_[opp j], term = 0, galpha = 0;  equilibrium cells: mu = 0 (term and galpha as above)
            6. mu is rounded to the store dtype; the transposed streaming is _adjoint_ref.stream_transpose
            7. the gradient field is fp64: dalpha += float64(galpha), step after step in the order of the sweep
"""

import numpy as np

from oracle import xlb_numpy as orc

import _adjoint_ref as adj


def _damped(fs, alpha, lat):
    T = fs.dtype.type
    rho1, u = orc.macroscopic(fs, lat)
    kappa = T(1.0) - alpha[0].astype(T)
    ut = np.empty_like(u)
    for d in range(lat.d):
        ut[d] = kappa * u[d]
    return rho1, u, kappa, ut


def step(f_0, alpha, bc_mask, missing_mask, bcs, omega, lat, policy="FP32FP32"):
    """One porous step -> f_1 (store dtype)"""
    adj._check(bcs)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    fs = adj.post_stream(f_0.astype(T), bc_mask, missing_mask, bcs, lat, policy)
    with np.errstate(all="ignore"):
        rho1, _, _, ut = _damped(fs, alpha, lat)
        out = orc.bgk(fs, orc.equilibrium(rho1, ut, lat, T), omega)
    for bc in bcs:
        if bc.step == orc.STEP_COLLISION:
            out = orc.apply_bc(bc, fs, out, bc_mask, missing_mask, lat, policy)
    return out.astype(S)


def run(f_0, alpha, bc_mask, missing_mask, bcs, omega, lat, n_steps, policy="FP32FP32"):
    f = f_0
    for _ in range(n_steps):
        f = step(f, alpha, bc_mask, missing_mask, bcs, omega, lat, policy)
    return f


def forward_states(f_0, alpha, bc_mask, missing_mask, bcs, omega, lat, n_steps, policy="FP32FP32"):
    """[f_0 .. f_{n-1}] and f_n"""
    states, f = [], f_0
    for _ in range(n_steps):
        states.append(f)
        f = step(f, alpha, bc_mask, missing_mask, bcs, omega, lat, policy)
    return states, f


def collide_transpose(fs, lam, alpha, omega, lat):
    """adjoint steps 2-4 for every cell: (mu, term, galpha)"""
    T = fs.dtype.type
    rho1, u, kappa, ut = _damped(fs, alpha, lat)
    rho = rho1[0]
    feq = orc.equilibrium(rho1, ut, lat, T)
    usq = ut[0] * ut[0]
    for d in range(1, lat.d):
        usq = usq + ut[d] * ut[d]
    usqr = T(1.5) * usq
    w = lat.w.astype(T)
    tu = [T(3.0) * ut[d] for d in range(lat.d)]
    A, B, term = None, [None] * lat.d, None
    for k in range(lat.q):
        cu = T(3.0) * adj._dot(ut, lat, k, T)
        e = (T(1.0) + cu * (T(1.0) + T(0.5) * cu)) - usqr
        a = lam[k] * (w[k] * e)
        A = a if A is None else A + a
        s = T(3.0) * (T(1.0) + cu)
        rw = rho * w[k]
        for d in range(lat.d):
            c = int(lat.c[d, k])
            g = s - tu[d] if c == 1 else ((-s) - tu[d] if c == -1 else -tu[d])
            b = lam[k] * (rw * g)
            B[d] = b if B[d] is None else B[d] + b
        t = lam[k] * (feq[k] - fs[k])
        term = t if term is None else term + t
    Br = [(kappa * B[d]) / rho for d in range(lat.d)]
    bu = B[0] * u[0]
    for d in range(1, lat.d):
        bu = bu + B[d] * u[d]
    om = T(omega)
    om1 = T(1.0) - om
    mu = np.empty_like(fs)
    for j in range(lat.q):
        acc = A
        for d in range(lat.d):
            acc = acc + Br[d] * adj._c_minus_u(int(lat.c[d, j]), u[d], T)
        mu[j] = om1 * lam[j] + om * acc
    return mu, term, -(om * bu)


def local_transpose(f_n, lam, alpha, bc_mask, missing_mask, bcs, omega, lat, policy):
    """adjoint steps 1-6a: mu in the store dtype, the per-cell omega terms and alpha terms (compute dtype)"""
    adj._check(bcs)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    fs = adj.post_stream(f_n.astype(T), bc_mask, missing_mask, bcs, lat, policy)
    L = lam.astype(T)
    with np.errstate(all="ignore"):
        mu, term, galpha = collide_transpose(fs, L, alpha, omega, lat)
    fw = adj._cells(bc_mask, bcs, orc.KIND_FULLWAY_BB)
    mu = np.where(fw[None], L[lat.opp], mu)
    term = np.where(fw, T(0), term)
    galpha = np.where(fw, T(0), galpha)
    mu = np.where(adj._cells(bc_mask, bcs, orc.KIND_EQUILIBRIUM)[None], T(0), mu)
    return mu.astype(S), term, galpha


def adjoint_step(f_n, lam, alpha, bc_mask, missing_mask, bcs, omega, lat, policy="FP32FP32"):
    """(lam_prev in the store dtype, per-cell omega terms, per-cell alpha terms; the terms in the compute dtype)"""
    mu, terms, galpha = local_transpose(f_n, lam, alpha, bc_mask, missing_mask, bcs, omega, lat, policy)
    return adj.stream_transpose(mu, bc_mask, missing_mask, bcs, lat, policy), terms, galpha


def backward(states, lam_final, alpha, bc_mask, missing_mask, bcs, omega, lat, policy="FP32FP32"):
    """The adjoint steps over states [f_0 .. f_{n-1}], last first -> (lam_0, [omega terms of step n-1, .. 0], dL/dalpha as the device
    accumulates it: fp64, shape (1,) + grid, step after step)"""
    lam, terms = lam_final, []
    dalpha = np.zeros(alpha.shape, dtype=np.float64)
    for f_n in reversed(states):
        lam, t, g = adjoint_step(f_n, lam, alpha, bc_mask, missing_mask, bcs, omega, lat, policy)
        terms.append(t)
        dalpha[0] = dalpha[0] + g.astype(np.float64)
    return lam, terms, dalpha


def gradient(f_0, alpha, bc_mask, missing_mask, bcs, omega, lat, n_steps, cotangent, policy="FP32FP32"):
    """(lam_0, [omega terms], dL/dalpha, f_n) of L(f_n); cotangent(f_n) -> lam_n in the store dtype"""
    states, f_n = forward_states(f_0, alpha, bc_mask, missing_mask, bcs, omega, lat, n_steps, policy)
    lam_0, terms, dalpha = backward(states, cotangent(f_n), alpha, bc_mask, missing_mask, bcs, omega, lat, policy)
    return lam_0, terms, dalpha, f_n


def tangent_step(f_n, v, alpha, dalpha, bc_mask, missing_mask, bcs, omega, lat, policy="FP64FP64", absolute=False):
    """Forward-mode twin: (dS/df_n) v + (dS/dalpha) dalpha, and with absolute=True the same chain of operations with every coefficient,
    v and dalpha replaced by its absolute value: an upper bound of the sum of the absolute products either side of the dot-product
    identity adds up."""
    adj._check(bcs)
    T = orc.compute_dtype(policy)
    ab = np.abs if absolute else (lambda x: x)
    fs = adj.post_stream(f_n.astype(T), bc_mask, missing_mask, bcs, lat, policy)
    V = ab(v.astype(T))
    da = ab(dalpha[0].astype(T))
    mm = missing_mask.astype(bool)
    eq, dn = adj._cells(bc_mask, bcs, orc.KIND_EQUILIBRIUM), adj._cells(bc_mask, bcs, orc.KIND_DO_NOTHING)
    hw, fw = adj._cells(bc_mask, bcs, orc.KIND_HALFWAY_BB), adj._cells(bc_mask, bcs, orc.KIND_FULLWAY_BB)
    dfs = orc.stream(V, lat)
    dfs = np.where(eq[None], T(0), dfs)
    dfs = np.where(dn[None], V, dfs)
    dfs = np.where(hw[None] & mm, V[lat.opp], dfs)
    rho1, u, kappa, ut = _damped(fs, alpha, lat)
    rho = rho1[0]
    usqr = T(1.5) * sum(ut[d] * ut[d] for d in range(lat.d))
    w = lat.w.astype(T)
    drho = sum(dfs[k] for k in range(lat.q))
    dut = []
    for d in range(lat.d):
        if absolute:
            du = (sum(abs(int(lat.c[d, k])) * dfs[k] for k in range(lat.q)) + np.abs(u[d]) * drho) / rho
            dut.append(np.abs(kappa) * du + np.abs(u[d]) * da)
        else:
            du = (sum(int(lat.c[d, k]) * dfs[k] for k in range(lat.q)) - u[d] * drho) / rho
            dut.append(kappa * du - u[d] * da)
    om = T(omega)
    out = np.empty_like(dfs)
    for k in range(lat.q):
        cu = T(3.0) * adj._dot(ut, lat, k, T)
        e = (T(1.0) + cu * (T(1.0) + T(0.5) * cu)) - usqr
        dfeq = ab(w[k] * e) * drho
        for d in range(lat.d):
            g = T(3.0) * int(lat.c[d, k]) * (T(1.0) + cu) - T(3.0) * ut[d]
            dfeq = dfeq + (rho * w[k]) * ab(g) * dut[d]
        out[k] = ab(T(1.0) - om) * dfs[k] + om * dfeq
    return np.where(fw[None], dfs[lat.opp], out)


def macroscopic_loss(f, u_target, lat, policy="FP64FP64"):
    """(L = 1/2 |u - u_target|^2 as a float, dL/du in the compute dtype) with the oracle's bare velocity u of f"""
    T = orc.compute_dtype(policy)
    _, u = orc.macroscopic(f.astype(T), lat)
    d = u - u_target.astype(T)
    return 0.5 * float(np.sum(d.astype(np.float64) ** 2)), d
