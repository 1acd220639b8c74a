"""NumPy restatement of the discrete adjoint of the fused BGK step (csrc/adjoint_kernels.hpp, adjoint_step_kernel.hpp).

TEST INFRASTRUCTURE ONLY.  The forward quantities come from the oracle's own operators (oracle/xlb_numpy.py: stream, apply_bc,
macroscopic, equilibrium); the transposed rules are stated here and pinned to the oracle's forward step by finite differences
(tests/test_adjoint_ref.py).  The reference differentiates its stepper through jax.grad and has no hand-written adjoint.

One forward step is f_{n+1} = S(f_n; omega) = oracle step with collision="BGK" and no force.  One adjoint step takes the forward state
f_n and the cotangent lam = dL/df_{n+1} and gives lam_prev = (dS/df_n)^T lam and the per-cell omega term.  The Jacobian is that of the
exact-arithmetic map (casts count as the identity).  In the compute dtype T, every sum sequential and no FMA:

  1. fs = pull stream of f_n + the streaming BCs (f*), rho, u, usqr and feq_k of fs as the oracle computes them
  2. per direction k = 0 .. q-1 (cu_k = 3 (c_k . u), e_k = (1 + cu_k (1 + 0.5 cu_k)) - usqr, s_k = 3 (1 + cu_k)):
         A    += lam_k (w_k e_k)
         B_d  += lam_k ((rho w_k) g_dk),  d ascending,  g_dk = s_k - 3 u_d | (-s_k) - 3 u_d | -(3 u_d)  for c_dk = 1 | -1 | 0
         term += lam_k (feq_k - fs_k)
     (the first term starts each sum)
  3. Br_d = B_d / rho;  mu_j = (1 - omega) lam_j + omega (A + sum_d Br_d (c_dj - u_d)),  the sum started at A, d ascending,
     c_dj - u_d = 1 - u_d | -1 - u_d | -u_d
  4. fullway cells: mu_j = lam_[opp j], term = 0;  equilibrium cells: mu = 0 (term as above)
  5. mu is rounded to the store dtype (the state the device carries between adjoint steps is mu in the store dtype)
  6. lam_prev_l(y) = gathered + own:  gathered = mu_l(y + c_l), periodic, or 0 where the forward pull of l at y + c_l was replaced
     (equilibrium and do-nothing cells: every l; halfway cells: their missing l);  own = mu_l(y) at a do-nothing cell,
     mu_[opp l](y) at a halfway cell that misses opp l, else nothing
  7. lam_prev is stored in the store dtype
"""

import numpy as np

from oracle import xlb_numpy as orc

SUPPORTED = (orc.KIND_EQUILIBRIUM, orc.KIND_HALFWAY_BB, orc.KIND_FULLWAY_BB, orc.KIND_DO_NOTHING)


def _check(bcs):
    for bc in bcs:
        if bc.kind not in SUPPORTED:
            raise NotImplementedError(f"adjoint restatement: bc kind {bc.kind}")


def _cells(bc_mask, bcs, kind):
    cells = np.zeros(bc_mask.shape[1:], dtype=bool)
    for bc in bcs:
        if bc.kind == kind:
            cells |= bc_mask[0] == bc.id
    return cells


def post_stream(F0, bc_mask, missing_mask, bcs, lat, policy):
    """f*: the oracle's stream and streaming-step BCs, in the order of its step"""
    fs = orc.stream(F0, lat)
    for bc in bcs:
        if bc.step == orc.STEP_STREAMING:
            fs = orc.apply_bc(bc, F0, fs, bc_mask, missing_mask, lat, policy)
    return fs


def _dot(u, lat, k, T):
    dot = np.zeros(u.shape[1:], dtype=T)
    for d in range(lat.d):
        cl = int(lat.c[d, k])
        if cl == 1:
            dot = dot + u[d]
        elif cl == -1:
            dot = dot - u[d]
    return dot


def _c_minus_u(c, ud, T):
    if c == 1:
        return T(1) - ud
    if c == -1:
        return T(-1) - ud
    return -ud


def collide_transpose(fs, lam, omega, lat):
    """steps 2 and 3 for every cell: (mu, term)"""
    T = fs.dtype.type
    rho1, u = orc.macroscopic(fs, lat)
    rho = rho1[0]
    feq = orc.equilibrium(rho1, u, lat, T)
    usq = u[0] * u[0]
    for d in range(1, lat.d):
        usq = usq + u[d] * u[d]
    usqr = T(1.5) * usq
    w = lat.w.astype(T)
    tu = [T(3.0) * u[d] for d in range(lat.d)]
    A, B, term = None, [None] * lat.d, None
    for k in range(lat.q):
        cu = T(3.0) * _dot(u, lat, k, T)
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
    Br = [B[d] / rho for d in range(lat.d)]
    om = T(omega)
    om1 = T(1.0) - om
    mu = np.empty_like(fs)
    for j in range(lat.q):
        acc = A
        for d in range(lat.d):
            acc = acc + Br[d] * _c_minus_u(int(lat.c[d, j]), u[d], T)
        mu[j] = om1 * lam[j] + om * acc
    return mu, term


def local_transpose(f_n, lam, bc_mask, missing_mask, bcs, omega, lat, policy):
    """steps 1-5: mu in the store dtype and the per-cell omega terms (compute dtype)"""
    _check(bcs)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    fs = post_stream(f_n.astype(T), bc_mask, missing_mask, bcs, lat, policy)
    L = lam.astype(T)
    with np.errstate(all="ignore"):
        mu, term = collide_transpose(fs, L, omega, lat)
    fw = _cells(bc_mask, bcs, orc.KIND_FULLWAY_BB)
    mu = np.where(fw[None], L[lat.opp], mu)
    term = np.where(fw, T(0), term)
    mu = np.where(_cells(bc_mask, bcs, orc.KIND_EQUILIBRIUM)[None], T(0), mu)
    return mu.astype(S), term


def stream_transpose(mu_s, bc_mask, missing_mask, bcs, lat, policy):
    """steps 6 and 7"""
    _check(bcs)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    mu = mu_s.astype(T)
    mm = missing_mask.astype(bool)
    eq, dn = _cells(bc_mask, bcs, orc.KIND_EQUILIBRIUM), _cells(bc_mask, bcs, orc.KIND_DO_NOTHING)
    hw = _cells(bc_mask, bcs, orc.KIND_HALFWAY_BB)
    blocked = (eq | dn)[None] | (hw[None] & mm)
    axes = tuple(range(lat.d))
    out = np.empty_like(mu)
    for l in range(lat.q):
        out[l] = np.roll(np.where(blocked[l], T(0), mu[l]), tuple(-int(s) for s in lat.c[:, l]), axis=axes)
    out = np.where(dn[None], out + mu, out)
    for l in range(lat.q):
        o = int(lat.opp[l])
        out[l] = np.where(hw & mm[o], out[l] + mu[o], out[l])
    return out.astype(S)


def adjoint_step(f_n, lam, bc_mask, missing_mask, bcs, omega, lat, policy="FP32FP32"):
    """(lam_prev in the store dtype, per-cell omega terms in the compute dtype)"""
    mu, terms = local_transpose(f_n, lam, bc_mask, missing_mask, bcs, omega, lat, policy)
    return stream_transpose(mu, bc_mask, missing_mask, bcs, lat, policy), terms


def forward_states(f_0, bc_mask, missing_mask, bcs, omega, lat, n_steps, policy="FP32FP32"):
    """[f_0 .. f_{n-1}] and f_n by the oracle's step"""
    states, f = [], f_0
    for _ in range(n_steps):
        states.append(f)
        f = orc.step(f, bc_mask, missing_mask, bcs, omega, lat, policy)
    return states, f


def backward(states, lam_final, bc_mask, missing_mask, bcs, omega, lat, policy="FP32FP32"):
    """The adjoint steps over states [f_0 .. f_{n-1}], last first -> (lam_0, [terms of step n-1, n-2, .. 0])"""
    lam, terms = lam_final, []
    for f_n in reversed(states):
        lam, t = adjoint_step(f_n, lam, bc_mask, missing_mask, bcs, omega, lat, policy)
        terms.append(t)
    return lam, terms


def tangent_step(f_n, v, bc_mask, missing_mask, bcs, omega, lat, policy="FP64FP64", absolute=False):
    """Forward-mode twin: (dS/df_n) v, and with absolute=True the same chain of operations with every coefficient and v replaced by
    its absolute value: an upper bound of the sum of the absolute products that either side of the dot-product identity adds up."""
    _check(bcs)
    T = orc.compute_dtype(policy)
    ab = np.abs if absolute else (lambda x: x)
    fs = post_stream(f_n.astype(T), bc_mask, missing_mask, bcs, lat, policy)
    V = ab(v.astype(T))
    mm = missing_mask.astype(bool)
    eq, dn = _cells(bc_mask, bcs, orc.KIND_EQUILIBRIUM), _cells(bc_mask, bcs, orc.KIND_DO_NOTHING)
    hw, fw = _cells(bc_mask, bcs, orc.KIND_HALFWAY_BB), _cells(bc_mask, bcs, orc.KIND_FULLWAY_BB)
    dfs = orc.stream(V, lat)
    dfs = np.where(eq[None], T(0), dfs)
    dfs = np.where(dn[None], V, dfs)
    dfs = np.where(hw[None] & mm, V[lat.opp], dfs)
    rho1, u = orc.macroscopic(fs, lat)
    rho = rho1[0]
    usqr = T(1.5) * sum(u[d] * u[d] for d in range(lat.d))
    w = lat.w.astype(T)
    drho = sum(dfs[k] for k in range(lat.q))
    du = []
    for d in range(lat.d):
        if absolute:
            du.append((sum(abs(int(lat.c[d, k])) * dfs[k] for k in range(lat.q)) + np.abs(u[d]) * drho) / rho)
        else:
            du.append((sum(int(lat.c[d, k]) * dfs[k] for k in range(lat.q)) - u[d] * drho) / rho)
    om = T(omega)
    out = np.empty_like(dfs)
    for k in range(lat.q):
        cu = T(3.0) * _dot(u, lat, k, T)
        e = (T(1.0) + cu * (T(1.0) + T(0.5) * cu)) - usqr
        dfeq = ab(w[k] * e) * drho
        for d in range(lat.d):
            g = T(3.0) * int(lat.c[d, k]) * (T(1.0) + cu) - T(3.0) * u[d]
            dfeq = dfeq + (rho * w[k]) * ab(g) * du[d]
        out[k] = ab(T(1.0) - om) * dfs[k] + om * dfeq
    return np.where(fw[None], dfs[lat.opp], out)


def omega_tangent(f_n, bc_mask, missing_mask, bcs, omega, lat, policy="FP64FP64"):
    """dS/domega at f_n: feq - f* outside the fullway cells"""
    T = orc.compute_dtype(policy)
    fs = post_stream(f_n.astype(T), bc_mask, missing_mask, bcs, lat, policy)
    rho1, u = orc.macroscopic(fs, lat)
    d = orc.equilibrium(rho1, u, lat, T) - fs
    return np.where(_cells(bc_mask, bcs, orc.KIND_FULLWAY_BB)[None], T(0), d)


def macroscopic_adjoint(f, rho_bar, u_bar, lat, policy="FP32FP32"):
    """dL/df_l = rho_bar + sum_d (u_bar_d / rho) (c_dl - u_d): the sum started at rho_bar, d ascending; stored in the store dtype"""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    rho1, u = orc.macroscopic(f.astype(T), lat)
    ur = [u_bar[d].astype(T) / rho1[0] for d in range(lat.d)]
    out = np.empty(f.shape, dtype=T)
    for l in range(lat.q):
        acc = rho_bar[0].astype(T)
        for d in range(lat.d):
            acc = acc + ur[d] * _c_minus_u(int(lat.c[d, l]), u[d], T)
        out[l] = acc
    return out.astype(S)
