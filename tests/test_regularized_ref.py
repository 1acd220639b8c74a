"""Closed-form pins for tests/_regularized_ref.py, the NumPy restatement of the regularised BGK collisions (fp64): conservation, the
relaxed stress, ghost modes, omega = 1, the third-order weights against their Gram-matrix derivation, and the viscosity of a decaying shear
wave against (1 / omega - 1 / 2) / 3 with BGK's own error on the same case as the yardstick (figures: profiles/regularized_collision.md)."""

import itertools

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _regularized_ref as ref

LATTICES = ("D2Q9", "D3Q19", "D3Q27")
OMEGA = 1.7
T = np.float64


def bc_shape(lat):
    return (-1,) + (1,) * lat.d


def random_state(lat, seed=3):
    """feq(rho, u) + eps with |u| <= 0.1 and eps ~ 1e-3 w"""
    rng = np.random.default_rng(seed)
    shape = (5,) * lat.d
    rho = 1.0 + 0.05 * rng.uniform(-1, 1, (1,) + shape)
    u = rng.uniform(-1, 1, (lat.d,) + shape)
    u *= 0.1 * rng.uniform(0, 1, shape) / np.sqrt((u * u).sum(axis=0))
    feq = orc.equilibrium(rho, u, lat, T)
    return feq + 1e-3 * lat.w.reshape(bc_shape(lat)) * rng.standard_normal(feq.shape)


def hermite_rows(lat, order):
    """the distinct Hermite polynomials of exactly this order on the lattice's velocities, {label: (q,)}; cs^2 = 1/3"""
    c = lat.c.astype(np.float64)
    rows = {}
    if order == 0:
        rows["1"] = np.ones(lat.q)
    elif order == 1:
        for a in range(lat.d):
            rows["xyz"[a]] = c[a]
    elif order == 2:
        for a, b in itertools.combinations_with_replacement(range(lat.d), 2):
            rows["xyz"[a] + "xyz"[b]] = c[a] * c[b] - (1.0 / 3.0 if a == b else 0.0)
    else:
        for a, b, g in itertools.combinations_with_replacement(range(lat.d), 3):
            h = c[a] * c[b] * c[g]
            # H_abg = c_a c_b c_g - cs^2 (c_a d_bg + c_b d_ag + c_g d_ab)
            h = h - (1.0 / 3.0) * (c[a] * (b == g) + c[b] * (a == g) + c[g] * (a == b))
            rows["xyz"[a] + "xyz"[b] + "xyz"[g]] = h
    return rows


def ghost_mode(lat, top_order, seed):
    """a vector orthogonal, under 1 / w, to w H for every Hermite polynomial of order <= top_order (third order: the lattice's components)"""
    rows = [h for o in range(top_order + 1) for h in hermite_rows(lat, o).values()]
    basis = np.array([lat.w * h for h in rows if np.abs(h).max() > 1e-12])  # the modes the collision keeps
    # orthogonal complement under <a, b> = sum a b / w: work with a / sqrt(w)
    s = np.sqrt(lat.w)
    _, sv, vt = np.linalg.svd(basis / s, full_matrices=True)
    null = vt[int((sv > 1e-10).sum()):]
    assert null.shape[0] > 0
    g = (np.random.default_rng(seed).standard_normal(null.shape[0]) @ null) * s
    assert np.abs((basis / lat.w) @ g).max() < 1e-14
    return g


@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", LATTICES)
def test_conserves_mass_and_momentum_and_relaxes_the_stress(lattice, form):
    lat = orc.Lattice(lattice)
    f = random_state(lat)
    rho, u = orc.macroscopic(f, lat)
    feq = orc.equilibrium(rho, u, lat, T)
    out = ref.collide(f, feq, u, OMEGA, lat, form)
    rho2, u2 = orc.macroscopic(out, lat)
    assert np.abs(rho2 - rho).max() <= 1e-13 * np.abs(rho).max()
    assert np.abs(rho2 * u2 - rho * u).max() <= 1e-13 * np.abs(rho * u).max()
    pi, pi2 = orc.second_moment(f - feq, lat), orc.second_moment(out - feq, lat)
    assert np.abs(pi).max() > 1e-5
    assert np.abs(pi2 - (1.0 - OMEGA) * pi).max() <= 1e-13 * np.abs(pi).max()


@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", LATTICES)
def test_annihilates_ghost_modes(lattice, form):
    lat = orc.Lattice(lattice)
    rng = np.random.default_rng(5)
    shape = (3,) * lat.d
    rho = 1.0 + 0.05 * rng.uniform(-1, 1, (1,) + shape)
    u = 0.05 * rng.uniform(-1, 1, (lat.d,) + shape)
    feq = orc.equilibrium(rho, u, lat, T)
    top = 3 if form == "RecursiveRegularizedBGK" else 2
    g = ghost_mode(lat, top, seed=11)
    # (the ghost carries no mass, momentum or stress, so rho, u and feq are those of feq alone)
    clean = ref.collide(feq, feq, u, OMEGA, lat, form)
    dirty = ref.collide(feq + 1e-3 * g.reshape(bc_shape(lat)), feq, u, OMEGA, lat, form)
    assert np.abs(dirty - clean).max() <= 1e-16
    # ... and BGK keeps it: the test would pass vacuously with g = 0
    kept = orc.bgk(feq + 1e-3 * g.reshape(bc_shape(lat)), feq, OMEGA) - orc.bgk(feq, feq, OMEGA)
    assert np.abs(kept).max() > 0.5 * 1e-3 * abs(1.0 - OMEGA) * np.abs(g).max() > 1e-7


@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", LATTICES)
def test_omega_one_returns_the_equilibrium(lattice, form):
    lat = orc.Lattice(lattice)
    f = random_state(lat, seed=8)
    rho, u = orc.macroscopic(f, lat)
    feq = orc.equilibrium(rho, u, lat, T)
    assert np.array_equal(ref.collide(f, feq, u, 1.0, lat, form), feq)


@pytest.mark.parametrize("lattice,rank", [("D2Q9", 2), ("D3Q19", 6), ("D3Q27", 7)])
def test_third_order_weights_follow_from_the_gram_matrix(lattice, rank):
    """f3 = W H^T G^+ a with G = H W H^T over the non-zero third-order Hermite components, each entering with its multiplicity in the
    symmetric tensor: the pseudo-inverse projection on their span.  The closed forms of the restatement must be that matrix."""
    lat = orc.Lattice(lattice)
    rows = {k: h for k, h in hermite_rows(lat, 3).items() if np.abs(h).max() > 1e-12}
    labels = ["xyz"[al] * 2 + "xyz"[be] for (al, be) in ref.aab_axes(lat)] + (["xyz"] if lat.d == 3 else [])
    labels = ["".join(sorted(s)) for s in labels]
    if lattice == "D3Q19":
        assert "xyz" not in rows
        labels = labels[:-1]
    assert sorted(rows) == sorted(labels)
    H = np.array([rows[k] for k in labels])
    G = (H * lat.w) @ H.T
    assert np.linalg.matrix_rank(G, tol=1e-12) == rank
    if lattice == "D3Q19":
        for p, q in ref.D3Q19_PAIRS:
            assert np.allclose(G[np.ix_([p, q], [p, q])] * 27.0, [[2, -1], [-1, 2]], atol=1e-13)
    derived = (lat.w[:, None] * H.T) @ np.linalg.pinv(G, rcond=1e-12)
    assert np.abs(derived - ref.third_order_weights(lat)).max() <= 1e-14


# ---- viscosity -----------------------------------------------------------------------------------------------------------------
SHEAR_CASES = [("D2Q9", (32, 32)), ("D3Q19", (32, 32, 4))]
SHEAR_OMEGA, SHEAR_STEPS, SHEAR_U0 = 1.6, 400, 0.01


def decay_rate_error(lat, shape, collision):
    """relative error of the fitted decay rate of ux = u0 sin(2 pi y / ny) against nu k^2, nu = (1 / omega - 1 / 2) / 3"""
    n = shape[1]
    y = (np.arange(n) + 0.5) / n
    u = np.zeros((lat.d,) + shape)
    u[0] = SHEAR_U0 * np.sin(2 * np.pi * y).reshape((1, n) + (1,) * (lat.d - 2))
    f = orc.equilibrium(np.ones((1,) + shape), u, lat, T)
    none_b, none_m = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    mode = np.sin(2 * np.pi * y).reshape((1, n) + (1,) * (lat.d - 2))
    amp, ts = [], []
    for t in range(SHEAR_STEPS + 1):
        if t >= 100 and t % 20 == 0:  # (after the start-up transient of the equilibrium initial state)
            _, uu = orc.macroscopic(f, lat)
            amp.append(2.0 * float((uu[0] * mode).mean()))
            ts.append(t)
        f = ref.step_any(f, none_b, none_m, [], SHEAR_OMEGA, lat, collision, "FP64FP64")
    rate = -np.polyfit(ts, np.log(amp), 1)[0]
    nu = (1.0 / SHEAR_OMEGA - 0.5) / 3.0
    return abs(rate / (nu * (2 * np.pi / n) ** 2) - 1.0)


@pytest.fixture(scope="module")
def shear_errors():
    return {(lattice, c): decay_rate_error(orc.Lattice(lattice), shape, c) for lattice, shape in SHEAR_CASES for c in ("BGK",) + ref.FORMS}


@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", [c[0] for c in SHEAR_CASES])
def test_shear_wave_viscosity(shear_errors, lattice, form):
    """The regularised forms get BGK's own error on the same case times 2 (the filter removes higher-order contributions BGK keeps)."""
    e_bgk, e = shear_errors[(lattice, "BGK")], shear_errors[(lattice, form)]
    print(f"{lattice}: decay-rate error BGK {e_bgk:.3e}, {form} {e:.3e}")
    assert e_bgk < 1e-2  # the case resolves the viscosity at all
    assert e <= 2.0 * e_bgk
