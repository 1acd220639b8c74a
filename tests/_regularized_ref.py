"""NumPy restatement of the regularised BGK collisions (xlb_amd/csrc/cell.hpp: regularized), on the oracle's lattices, dtypes and step.

    Pi_ab   = sum_l c_la c_lb (f_l - feq_l)                                     (oracle.second_moment of fneq)
    f1_l    = 4.5 w_l sum_ab (c_la c_lb - delta_ab / 3) Pi_ab                   (Latt and Chopard 2006)
    a_aab   = 2 u_a Pi_ab + u_b Pi_aa,   a_xyz = u_x Pi_yz + u_y Pi_xz + u_z Pi_xy   (Malaspinas 2015)
    f3_l    = w_l [13.5 sum_{a != b} H_aab,l a_aab + 27 H_xyz,l a_xyz]           (D2Q9, D3Q27)
    f3_l    = w_l sum_pairs [13.5 (H_p + H_q)_l (a_p + a_q) + 4.5 (H_p - H_q)_l (a_p - a_q)]   (D3Q19)
    f'_l    = feq_l + (1 - omega) (f1_l [+ f3_l])

with H_aab,l = (c_la^2 - 1/3) c_lb, H_xyz,l = c_lx c_ly c_lz and the D3Q19 pairs (xxy, yzz), (xxz, yyz), (xyy, xzz).  "RegularizedBGK" stops
at f1, "RecursiveRegularizedBGK" adds f3.  Every weight of f3 is 4.5 w_l times an integer (13.5 H_aab = 4.5 (3 c_a^2 - 1) c_b,
27 H_xyz = 4.5 * 6 c_x c_y c_z), which is how both this file and the device code form the constants.

The operations are written in the order of the device code so that results can be compared bit for bit in fp32 and fp64: sequential sums, no
fused multiply-adds, constants formed in double and rounded once to the compute dtype.  tests/test_regularized_ref.py pins this file to closed
forms (conservation, the stress, ghost modes, the Gram-matrix derivation of the third-order weights, the viscosity)."""

import numpy as np

from oracle import xlb_numpy as orc

FORMS = ("RegularizedBGK", "RecursiveRegularizedBGK")
D3Q19_PAIRS = ((0, 5), (1, 3), (2, 4))  # slots in aab_axes' order: (xxy, yzz), (xxz, yyz), (xyy, xzz)


def aab_axes(lat):
    """(alpha, beta) of the carried a_aab, alpha-major over alpha != beta: xxy, xxz, xyy, yyz, xzz, yzz (2-D: xxy, xyy)"""
    return [(al, be) for al in range(lat.d) for be in range(lat.d) if al != be]


def pi_slot(lat, a, b):
    a, b = min(a, b), max(a, b)
    return [(i, j) for i in range(lat.d) for j in range(i, lat.d)].index((a, b))


def qi(lat):
    """(q, n_pi) doubles: c_a c_b - 1/3 on the diagonal components, 2 c_a c_b off the diagonal (cell.hpp qi)"""
    out = np.zeros_like(lat.cc)
    for k, (a, b) in enumerate((i, j) for i in range(lat.d) for j in range(i, lat.d)):
        for l in range(lat.q):
            out[l, k] = float(lat.cc[l, k]) - 1.0 / 3.0 if a == b else float(lat.cc[l, k]) * 2.0
    return out


def n3(lat):
    """(q, n_carried) integers: weight of each carried third-order value in f3_l, in units of 4.5 w_l (cell.hpp n3).  Carried values: the
    a_aab and a_xyz themselves (D2Q9, D3Q27), or the sums and differences of the three pairs (D3Q19: s0, d0, s1, d1, s2, d2)."""
    c = lat.c
    h3 = np.array([[(3 * int(c[al, l]) ** 2 - 1) * int(c[be, l]) for (al, be) in aab_axes(lat)] for l in range(lat.q)])  # 3 H_aab
    if lat.name == "D3Q19":
        cols = []
        for p, q in D3Q19_PAIRS:
            cols += [h3[:, p] + h3[:, q], (h3[:, p] - h3[:, q]) // 3]
        assert all(((h3[:, p] - h3[:, q]) % 3 == 0).all() for p, q in D3Q19_PAIRS)
        return np.stack(cols, axis=1)
    if lat.name == "D3Q27":
        return np.concatenate([h3, (6 * c[0] * c[1] * c[2])[:, None]], axis=1)
    return h3


def third_order_weights(lat):
    """f3 = K a as a (q, n_aab [+ 1]) float64 matrix on the PLAIN components (a_aab in aab_axes' order, then a_xyz in 3-D): what the
    closed forms above say, for comparison with the Gram-matrix derivation"""
    n = n3(lat).astype(np.float64)
    k = 4.5 * lat.w[:, None] * n
    if lat.name != "D3Q19":
        return k
    out = np.zeros((lat.q, 6))
    for i, (p, q) in enumerate(D3Q19_PAIRS):
        out[:, p] += k[:, 2 * i] + k[:, 2 * i + 1]  # s = a_p + a_q, d = a_p - a_q
        out[:, q] += k[:, 2 * i] - k[:, 2 * i + 1]
    return out


def third_moment(u, pi, lat):
    """the carried third-order values of n3(), each (nx, ny[, nz]) in the dtype of u"""
    T = u.dtype.type
    aab = [(T(2.0) * u[al]) * pi[pi_slot(lat, al, be)] + u[be] * pi[pi_slot(lat, al, al)] for (al, be) in aab_axes(lat)]
    if lat.name == "D3Q19":
        out = []
        for p, q in D3Q19_PAIRS:
            out += [aab[p] + aab[q], aab[p] - aab[q]]
        return out
    if lat.name == "D3Q27":
        aab.append((u[0] * pi[4] + u[1] * pi[2]) + u[2] * pi[1])
    return aab


def hermite2(pi, lat):
    """f1: (q, ...) from Pi (n_pi, ...)"""
    T = pi.dtype.type
    q2, w = qi(lat), lat.w.astype(T)
    out = np.empty((lat.q,) + pi.shape[1:], dtype=pi.dtype)
    for l in range(lat.q):
        qp = T(q2[l, 0]) * pi[0]
        for k in range(1, pi.shape[0]):
            qp = qp + T(q2[l, k]) * pi[k]
        out[l] = (T(4.5) * w[l]) * qp
    return out


def collide(f, feq, u, omega, lat, form):
    """f' from the post-streaming populations f, their equilibrium feq and velocity u (all in the compute dtype)"""
    assert form in FORMS
    T = f.dtype.type
    pi = orc.second_moment(f - feq, lat)
    r = hermite2(pi, lat)
    if form == "RecursiveRegularizedBGK":
        a, n = third_moment(u, pi, lat), n3(lat)
        for l in range(lat.q):
            for j in range(n.shape[1]):
                if n[l, j] != 0:
                    r[l] = r[l] + T(4.5 * float(lat.w[l]) * int(n[l, j])) * a[j]
    keep = T(1.0) - T(omega)
    return feq + keep * r


def collide_from_f(f, omega, lat, form):
    """the stand-alone operator's arithmetic with feq = equilibrium(moments of f)"""
    rho, u = orc.macroscopic(f, lat)
    return collide(f, orc.equilibrium(rho, u, lat, f.dtype.type), u, omega, lat, form)


def step(f_0, bc_mask, missing_mask, bcs, omega, lat, form, policy="FP32FP32", force_vector=None):
    """oracle.step with the regularised collision in the collision's place"""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    F0 = f_0.astype(T)
    post_stream = orc.stream(F0, lat)
    for bc in bcs:
        if bc.step == orc.STEP_STREAMING:
            post_stream = orc.apply_bc(bc, F0, post_stream, bc_mask, missing_mask, lat, policy)
    rho, u = orc.macroscopic(post_stream, lat)
    feq = orc.equilibrium(rho, u, lat, T)
    post_coll = collide(post_stream, feq, u, omega, lat, form)
    if force_vector is not None:
        post_coll = orc.exact_difference_force(post_coll, feq, lat, force_vector)
    for bc in bcs:
        post_coll = orc.assemble_auxiliary_data(bc, post_stream, post_coll, bc_mask, missing_mask, lat)
        if bc.step == orc.STEP_COLLISION:
            post_coll = orc.apply_bc(bc, post_stream, post_coll, bc_mask, missing_mask, lat, policy)
    return post_coll.astype(S)


def run(f_0, bc_mask, missing_mask, bcs, omega, lat, form, n_steps, policy="FP32FP32", force_vector=None):
    f = f_0
    for _ in range(n_steps):
        f = step(f, bc_mask, missing_mask, bcs, omega, lat, form, policy, force_vector)
    return f


def step_any(f_0, bc_mask, missing_mask, bcs, omega, lat, collision, policy="FP32FP32", force_vector=None):
    """one step with a regularised form or one of the oracle's own collisions"""
    if collision in FORMS:
        return step(f_0, bc_mask, missing_mask, bcs, omega, lat, collision, policy, force_vector)
    return orc.step(f_0, bc_mask, missing_mask, bcs, omega, lat, policy, collision, force_vector)


# ---- the cases the tests share ---------------------------------------------------------------------------------------------------
def sheared_state(shape, lat, policy, u0=0.04):
    """an equilibrium with a sheared, divergence-carrying velocity field and a density ripple: Pi and u are non-trivial from step one"""
    T = orc.compute_dtype(policy)
    x = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    u = np.zeros((lat.d,) + tuple(shape))
    u[0] = u0 * np.sin(2 * np.pi * x[1]) + 0.3 * u0 * np.cos(2 * np.pi * x[0])
    u[1] = 0.5 * u0 * np.sin(2 * np.pi * (x[0] + 0.25)) * np.cos(2 * np.pi * x[1])
    if lat.d == 3:
        u[2] = 0.4 * u0 * np.sin(2 * np.pi * (x[2] + x[0]))
        u[0] += 0.2 * u0 * np.cos(2 * np.pi * x[2])
    rho = 1.0 + 0.02 * np.cos(2 * np.pi * (x[0] - x[1]))
    return orc.equilibrium(rho[None].astype(T), u.astype(T), lat, T).astype(orc.store_dtype(policy))


def double_shear_layer(shape, lat, policy, u0=0.04):
    """the double shear layer of Minion and Brown at cell centres: ux = u0 tanh(80 (y - 1/4)) for y <= 1/2, u0 tanh(80 (3/4 - y)) above;
    uy = 0.05 u0 sin(2 pi (x + 1/4)); in 3-D uz = 0.05 u0 sin(2 pi (z + x)).  rho = 1"""
    T = orc.compute_dtype(policy)
    x = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in shape], indexing="ij")
    u = np.zeros((lat.d,) + tuple(shape))
    u[0] = np.where(x[1] <= 0.5, u0 * np.tanh(80.0 * (x[1] - 0.25)), u0 * np.tanh(80.0 * (0.75 - x[1])))
    u[1] = 0.05 * u0 * np.sin(2 * np.pi * (x[0] + 0.25))
    if lat.d == 3:
        u[2] = 0.05 * u0 * np.sin(2 * np.pi * (x[2] + x[0]))
    rho = np.ones((1,) + tuple(shape))
    return orc.equilibrium(rho.astype(T), u.astype(T), lat, T).astype(orc.store_dtype(policy))


def max_speed(f, lat):
    """max |u| of a population field; inf when anything is not finite"""
    f = np.asarray(f, dtype=np.float64)
    if not np.isfinite(f).all():
        return float("inf")
    _, u = orc.macroscopic(f, lat)
    m = float(np.sqrt((u * u).sum(axis=0)).max())
    return m if np.isfinite(m) else float("inf")
