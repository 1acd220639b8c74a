"""NumPy restatement of the reference's immersed-boundary coupling (xlb/operator/stepper/ibm_stepper.py), test infrastructure only.

Everything is computed in the policy's COMPUTE dtype with sequential sums (markers in array order per cell, cells in x, y, z order
per marker), on top of oracle.xlb_numpy's ``step``, ``macroscopic`` and ``equilibrium``.  The hash grid of the reference is a
neighbour search only: a marker's candidates are the cells with |r| <= 2 per axis inside the box (no periodic wrap).
"""

import numpy as np

from oracle import xlb_numpy as orc


def peskin_weight(r, T):
    """ibm_stepper.py:158-173"""
    a = np.abs(np.asarray(r, dtype=T))
    with np.errstate(invalid="ignore"):
        inner = T(0.125) * ((T(3) - T(2) * a) + np.sqrt((T(1) + T(4) * a) - (T(4) * a) * a))
        outer = T(0.125) * ((T(5) - T(2) * a) - np.sqrt((T(-7) + T(12) * a) - (T(4) * a) * a))
    return np.where(a <= T(1), inner, np.where(a <= T(2), outer, T(0))).astype(T)


def support(X, shape, T):
    """Cells (m, 3) with |r| <= 2 per axis inside the box and their weights (m,), ibm_stepper.py:176-178 with the cell (i, j, k) at
    (i + 1/2, j + 1/2, k + 1/2) (:105); x slowest, z fastest."""
    X = np.asarray(X, dtype=np.float32).astype(T)
    axes, weights = [], []
    for a in range(3):
        lo = max(int(np.ceil(float(X[a]) - 2.5)), 0)
        hi = min(int(np.floor(float(X[a]) + 1.5)), shape[a] - 1)
        i = np.arange(lo, hi + 1)
        r = (i.astype(T) + T(0.5)) - X[a]
        keep = np.abs(r) <= T(2)
        axes.append(i[keep])
        weights.append(peskin_weight(r[keep], T))
    ii, jj, kk = np.meshgrid(*axes, indexing="ij")
    wx, wy, wz = np.meshgrid(*weights, indexing="ij")
    w = ((wx * wy) * wz).astype(T)
    return np.stack([ii.ravel(), jj.ravel(), kk.ravel()], axis=1), w.ravel()


def _pairs(positions, shape, T):
    """(marker index, linear cell index, weight) of every marker-cell pair, marker-major."""
    ks, cs, ws = [], [], []
    for k, X in enumerate(np.asarray(positions, dtype=np.float32)):
        cells, w = support(X, shape, T)
        lin = (cells[:, 0] * shape[1] + cells[:, 1]) * shape[2] + cells[:, 2]
        ks.append(np.full(lin.shape, k))
        cs.append(lin)
        ws.append(w)
    if not ks:
        z = np.zeros(0, dtype=np.int64)
        return z, z, np.zeros(0, dtype=T)
    return np.concatenate(ks), np.concatenate(cs), np.concatenate(ws)


def couple(f_1, positions, areas, velocities, lat, policy, max_iterations=4, tolerance=1e-5, relaxation=1.0):
    """The coupling of ibm_stepper.py:391-476 on f_1 (store dtype) -> dict(f=f_1 after, forces (n, 3), sweeps, G (3, ...), W (...))."""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    shape = f_1.shape[1:]
    n = len(positions)
    rho, u = orc.macroscopic(f_1.astype(T), lat)
    uc = u.reshape(3, -1)  # (3, cells)
    k_of, c_of, w_of = _pairs(positions, shape, T)
    A = np.asarray(areas, dtype=np.float32).astype(T)
    U = np.asarray(velocities, dtype=np.float32).astype(T).reshape(n, 3)
    F = np.zeros((n, 3), dtype=T)
    G = np.zeros((3, uc.shape[1]), dtype=T)
    W = np.zeros(uc.shape[1], dtype=T)
    tol_sq = T(tolerance * tolerance)
    sweeps, flag_pending, flag = 0, False, False
    for it in range(max_iterations):
        if flag_pending:  # :413-419
            flag_pending = False
            if not flag:
                break
        prev = F.copy()
        acc = np.zeros((3, uc.shape[1]), dtype=T)
        W = np.zeros(uc.shape[1], dtype=T)
        np.add.at(W, c_of, w_of)  # (ufunc.at adds one element after the other, in array order)
        for a in range(3):
            np.add.at(acc[a], c_of, (F[k_of, a] * w_of) * A[k_of])  # :283-293
        with np.errstate(all="ignore"):
            G = np.where(W > T(0), T(relaxation) * (acc / W - uc), acc).astype(T)  # :320-325
        num = np.zeros((n, 3), dtype=T)
        den = np.zeros(n, dtype=T)
        for a in range(3):
            np.add.at(num[:, a], k_of, uc[a, c_of] * w_of)  # :349-354
        np.add.at(den, k_of, w_of)
        with np.errstate(all="ignore"):
            u_interp = np.where(den[:, None] > T(0), num / den[:, None], T(0)).astype(T)
        F = F + (U - u_interp)  # :361-362
        sweeps = it + 1
        if it > 0 and tolerance > 0:  # :364-368, :446
            diff = F - prev
            sq = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
            flag = bool(np.any(sq > tol_sq))
            flag_pending = True
    Gf = G.reshape((3,) + shape)
    feq_force = orc.equilibrium(rho, u + Gf, lat, T)
    feq = orc.equilibrium(rho, u, lat, T)
    out = f_1 + (feq_force - feq).astype(S)  # :261 (the sum is taken in the store dtype)
    return {"f": out.astype(S), "forces": F, "sweeps": sweeps, "G": Gf, "W": W.reshape(shape)}


def step(f_0, positions, areas, velocities, bc_mask, missing_mask, bcs, omega, lat, policy, collision, **ibm):
    """One IBMStepper call: the fluid step, then the coupling on its result."""
    with np.errstate(all="ignore"):
        f_1 = orc.step(f_0, bc_mask, missing_mask, bcs, omega, lat, policy, collision)
    return couple(f_1, positions, areas, velocities, lat, policy, **ibm)


def fibonacci_sphere(n, radius, centre):
    """n points on a sphere (golden-angle spiral), float32 (n, 3)."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = np.pi * (3.0 - np.sqrt(5.0)) * k
    s = np.sqrt(1.0 - z * z)
    p = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1) * radius + np.asarray(centre, dtype=np.float64)
    return p.astype(np.float32)
