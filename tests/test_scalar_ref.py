"""Physics pins of the scalar-transport restatement (tests/_scalar_ref.py), on the CPU.

The reference has no scalar transport to compare with, so the restatement — which the host emulation and the GPU tests are compared
with — is pinned by closed-form solutions and conservation.  Every bound is TWICE the figure measured with this restatement
(MEASURED below, also in profiles/scalar_transport.md): the factor 2 covers the rounding scatter of another summation order (NumPy's
pairwise sums in the diagnostics), nothing more.  A measured 0 is asserted as 0."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _scalar_ref as ref

# (check, dimension, policy) -> figure measured with the committed restatement
MEASURED = {
    ("sine", 3, "FP64FP64"): 1.6668e-04, ("sine", 3, "FP32FP32"): 1.6882e-04,
    ("sine", 2, "FP64FP64"): 1.0023e-04, ("sine", 2, "FP32FP32"): 1.0745e-04,
    ("conduction", 3, "FP64FP64"): 1.6653e-15, ("conduction", 3, "FP32FP32"): 8.9407e-07,
    ("conduction", 2, "FP64FP64"): 2.3315e-15, ("conduction", 2, "FP32FP32"): 7.7486e-07,
    ("drift_plates", 3, "FP64FP64"): 1.4578e-16, ("drift_plates", 3, "FP32FP32"): 1.6447e-07,
    ("drift_plates", 2, "FP64FP64"): 1.5009e-14, ("drift_plates", 2, "FP32FP32"): 7.8548e-06,
    ("drift_periodic", 3, "FP64FP64"): 0.0, ("drift_periodic", 3, "FP32FP32"): 1.7199e-06,
    ("drift_periodic", 2, "FP64FP64"): 1.8430e-14, ("drift_periodic", 2, "FP32FP32"): 7.3379e-06,
}
CASES = [(d, p) for d in (3, 2) for p in ("FP64FP64", "FP32FP32")]


def lattice(dim):
    return orc.Lattice("D3Q19" if dim == 3 else "D2Q9")


def no_walls(shape, lat):
    return np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)


def plates(shape, lat):
    """Halfway walls below the first and above the last cell of the last axis, ids 1 (bottom) and 2 (top), periodic sides.  The masks
    are written by hand: the masker also flags the directions that leave the box sideways at the plates' edge cells, which would put
    a piece of wall there and spoil the one-dimensional solutions these pins compare with."""
    bm, mm = no_walls(shape, lat)
    bm[0][..., 0], bm[0][..., -1] = 1, 2
    for l in range(lat.q):
        mm[l][..., 0] = lat.c[-1, l] == 1
        mm[l][..., -1] = lat.c[-1, l] == -1
    return bm, mm


def total(g):
    """total scalar, summed in fp64 (a diagnostic: its order is not the kernels')"""
    return float(g.astype(np.float64).sum())


def sine_mode(dim, policy, steps=200):
    """A sine mode of amplitude 0.1 on a mean of 1 carried by a uniform flow u_x = 0.05, omega_s = 1.25:
    phi = 1 + 0.1 exp(-D k^2 t) sin(k (x + 1/2 - u t)).  Returns (max error, remaining amplitude, relative drift of the total)."""
    lat = lattice(dim)
    sl = ref.ScalarLattice(lat)
    T = orc.compute_dtype(policy)
    shape = (32, 4, 4) if dim == 3 else (32, 4)
    omega_s, ux, amp = 1.25, 0.05, 0.1
    k = 2 * np.pi / shape[0]
    x = np.arange(shape[0]).reshape((-1,) + (1,) * (dim - 1)) + 0.5
    phi0 = np.broadcast_to(1.0 + amp * np.sin(k * x), shape)
    u = np.zeros((dim,) + shape, T)
    u[0] = T(ux)
    g = ref.equilibrium_g(phi0.astype(T), u, sl, T).astype(orc.store_dtype(policy))
    bm, mm = no_walls(shape, lat)
    t0 = total(g)
    for _ in range(steps):
        g = ref.scalar_step(g, u, bm, mm, [], omega_s, lat, policy)
    decay = np.exp(-sl.diffusivity(omega_s) * k * k * steps)
    exact = 1.0 + amp * decay * np.sin(k * (x - ux * steps))
    phi = ref.moment(g, policy)[0].astype(np.float64)
    return float(np.abs(phi - exact).max()), float(amp * decay), abs(total(g) - t0) / abs(t0)


def conduction(dim, policy, steps=3000):
    """Two Dirichlet plates (1 below, 0 above), fluid at rest, omega_s = 1: phi(z) = 1 - (z + 1/2) / nz.  Returns the maximum error."""
    lat = lattice(dim)
    shape = (3, 4, 8) if dim == 3 else (4, 8)
    nz = shape[-1]
    bm, mm = plates(shape, lat)
    rules = [ref.Rule(ref.DIRICHLET, 1, 1.0), ref.Rule(ref.DIRICHLET, 2, 0.0)]
    T = orc.compute_dtype(policy)
    u = np.zeros((dim,) + shape, T)
    g = ref.equilibrium_g(np.full(shape, 0.5, T), u, ref.ScalarLattice(lat), T).astype(orc.store_dtype(policy))
    for _ in range(steps):
        g = ref.scalar_step(g, u, bm, mm, rules, 1.0, lat, policy)
    exact = 1.0 - (np.arange(nz) + 0.5) / nz
    return float(np.abs(ref.moment(g, policy)[0].astype(np.float64) - exact).max())


def drift_plates(dim, policy, steps=200):
    """Relative drift of the total scalar between two ADIABATIC plates, random field, fluid at rest."""
    lat = lattice(dim)
    shape = (3, 4, 8) if dim == 3 else (4, 8)
    bm, mm = plates(shape, lat)
    T = orc.compute_dtype(policy)
    u = np.zeros((dim,) + shape, T)
    phi0 = np.random.default_rng(3).uniform(0.5, 1.5, shape).astype(T)
    g = ref.equilibrium_g(phi0, u, ref.ScalarLattice(lat), T).astype(orc.store_dtype(policy))
    t0 = total(g)
    for _ in range(steps):
        g = ref.scalar_step(g, u, bm, mm, [], 1.3, lat, policy)
    return abs(total(g) - t0) / abs(t0)


def figure(check, dim, policy):
    if check == "sine":
        return sine_mode(dim, policy)[0]
    if check == "conduction":
        return conduction(dim, policy)
    if check == "drift_plates":
        return drift_plates(dim, policy)
    return sine_mode(dim, policy)[2]


@pytest.mark.parametrize("check", ["sine", "conduction", "drift_plates", "drift_periodic"])
@pytest.mark.parametrize("dim,policy", CASES)
def test_physics_pin(check, dim, policy):
    got = figure(check, dim, policy)
    bound = 2.0 * MEASURED[(check, dim, policy)]
    print(f"{check} D{dim} {policy}: measured {got:.4e}, bound {bound:.4e}")
    assert got <= bound


def test_sine_mode_has_decayed_to_the_amplitude_of_the_closed_form():
    err, amplitude, _ = sine_mode(3, "FP64FP64")
    assert abs(amplitude - 0.056) < 5e-4 and err < 0.01 * amplitude


def test_scalar_directions_are_the_main_indices_in_ascending_order():
    assert ref.ScalarLattice(orc.Lattice("D3Q19")).dirs.tolist() == [0, 1, 2, 3, 6, 9, 14]
    for name in ("D2Q9", "D3Q19", "D3Q27"):
        lat = orc.Lattice(name)
        sl = ref.ScalarLattice(lat)
        assert sl.q == 2 * lat.d + 1 and np.array_equal(sl.c[:, sl.opp], -sl.c)
        assert abs(sl.w.sum() - 1.0) < 1e-15
        second = (sl.w * sl.c[:, None, :] * sl.c[None, :, :]).sum(axis=2)  # sum_j w_j c_j c_j = cs^2 I
        assert np.allclose(second, sl.cs2 * np.eye(lat.d), atol=1e-15)


@pytest.mark.parametrize("lattice_name,policy", [("D3Q19", "FP32FP32"), ("D3Q19", "FP64FP64"), ("D2Q9", "FP64FP64")])
def test_uniform_scalar_excess_acts_like_a_force_vector(lattice_name, policy):
    """A uniform phi = reference + delta in a periodic box must accelerate the fluid like force_vector = buoyancy * delta."""
    lat = orc.Lattice(lattice_name)
    shape = (6, 5, 4)[: lat.d]
    T = orc.compute_dtype(policy)
    buoyancy = np.array([0.0, 0.0, 2e-3])[-lat.d :] if lat.d == 3 else np.array([0.0, 2e-3])
    reference, delta, steps = 0.5, 0.25, 5
    bm, mm = no_walls(shape, lat)
    f = orc.initialize_eq(shape, lat, policy)  # (at rest: phi stays uniform; a non-solenoidal flow would compress it)
    g = ref.init_g(reference + delta, f, lat, policy)
    f_s, g_s = ref.run(f, g, bm, mm, [], [], 1.1, 1.3, lat, steps, policy=policy, buoyancy=buoyancy, reference=reference)
    f_o = orc.run(f, bm, mm, [], 1.1, lat, steps, policy, "BGK", force_vector=buoyancy * delta)
    rho_s, u_s = orc.macroscopic(f_s.astype(T), lat)
    rho_o, u_o = orc.macroscopic(f_o.astype(T), lat)
    figures = (np.abs(rho_s.astype(float) - rho_o).max(), np.abs(u_s.astype(float) - u_o).max())
    print(lattice_name, policy, "max |d rho| %.2e  |d u| %.2e" % figures)
    assert max(figures) <= 1e-6
    assert np.abs(u_o.astype(float)[-1].mean() - orc.macroscopic(f.astype(T), lat)[1].astype(float)[-1].mean()) > 1e-3  # the force did act
