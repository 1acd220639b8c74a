"""Physics pins of the NumPy restatement of the two-component Shan-Chen step (tests/_multicomponent_ref.py): what the scheme must do
whatever code runs it.  FP64FP64 on D2Q9.  Every bound is twice the figure measured with the committed restatement (MEASURED below,
recorded in profiles/multicomponent.md); each test prints its figure before it asserts.  The layered Poiseuille flow with a viscosity
contrast is measured and printed, not asserted (see its docstring)."""

import functools
import math

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _multicomponent_cases as cases
import _multicomponent_ref as ref

POLICY = "FP64FP64"
LAT = orc.Lattice("D2Q9")
G_SEPARATING = 2.4  # G_AB of the separated states (droplets, slabs, layers); G_AA = G_BB = 0
RHO_MAJOR, RHO_MINOR = 1.0, 0.04  # start densities of a component where it is the majority and where it is the minority

# the figures of the committed restatement; asserted at twice each
MEASURED = {
    "force_sum": 9.888e-17,  # max |sum_x (F^A + F^B)_a| over four random fields (math.fsum), max |F^A + F^B| = 0.174
    "momentum_drift_50": 1.581e-18,  # |P(50) - P(0)| / mass, exact sums
    "mass_drift_periodic": 3.958e-13,  # relative, either component, 6000 steps, the slab of A in B
    "mass_drift_walled": 1.581e-13,  # relative, either component, 3000 steps, the sessile droplet between neutral plates
    "reduction_distance": 2.220e-16,  # max |f^A + f^B - f| after 20 steps of the oracle's BGK step, all G = 0
    "laplace_spread": 8.418e-03,  # (max - min) / mean of (p_in - p_out) R = 0.14933, 0.14823, 0.14949 (max |u| 0.024, 0.020, 0.022)
}


def bound(key):
    return 2.0 * MEASURED[key]


def total_mass(f):
    """exactly rounded, so that a drift is the scheme's and not the sum's"""
    return math.fsum(f.astype(np.float64).ravel())


def total_momentum(*fs):
    c = [LAT.c[a][(slice(None),) + (None,) * LAT.d] for a in range(LAT.d)]
    return np.array([math.fsum(np.concatenate([(c[a] * f.astype(np.float64)).ravel() for f in fs])) for a in range(LAT.d)])


def separating():
    return ref.Mixture(G_SEPARATING)


def parts_of(fa, fb, bm, mm, bcs, mix, wall_density=None):
    return ref.outputs(fa, fb, bm, mm, bcs, LAT, mix, wall_density, POLICY)


def at_rest(rho_a, rho_b):
    return ref.init_at_rest(rho_a, LAT, POLICY), ref.init_at_rest(rho_b, LAT, POLICY)


def two_sided(profile):
    """profile in [0, 1] -> (rho_A, rho_B): A the majority where it is 1, B where it is 0"""
    return RHO_MINOR + (RHO_MAJOR - RHO_MINOR) * profile, RHO_MINOR + (RHO_MAJOR - RHO_MINOR) * (1.0 - profile)


# ---- momentum ------------------------------------------------------------------------------------------------------------------------
def random_rest_state(seed):
    shape = (16, 12)
    rng = np.random.default_rng(seed)
    return shape, at_rest(rng.uniform(0.1, 1.5, shape), rng.uniform(0.1, 1.5, shape))


def test_the_two_forces_sum_to_zero_over_a_periodic_box():
    """the cross terms cancel in pairs (x, x + c_i), and so do the self terms of G_AA and G_BB"""
    mix = cases.mixture()
    worst, largest = 0.0, 0.0
    for seed in range(4):
        shape, (fa, fb) = random_rest_state(seed)
        bm, mm = ref.no_walls(shape, LAT)
        parts = parts_of(fa, fb, bm, mm, [], mix)
        total = parts["force_a"] + parts["force_b"]
        worst = max(worst, max(abs(math.fsum(total[a].ravel())) for a in range(LAT.d)))
        largest = max(largest, float(np.abs(total).max()))
    print(f"max |sum_x (F^A + F^B)| = {worst:.3e} with max |F^A + F^B| = {largest:.3e}")
    assert largest > 0.1
    assert worst <= bound("force_sum")


def test_total_momentum_stays_put_over_fifty_steps():
    """unequal relaxation rates: the collision conserves the total momentum only through the omega-weighted common velocity"""
    mix = cases.mixture()
    shape = (16, 12)
    fa, fb = cases.random_states(shape, LAT, POLICY, seed=3)
    bm, mm = ref.no_walls(shape, LAT)
    p0 = total_momentum(fa, fb)
    assert np.abs(p0).max() > 1e-2
    fa, fb = ref.run(fa, fb, bm, mm, [], cases.OMEGA, LAT, mix, 50, policy=POLICY)
    assert np.isfinite(fa).all() and np.isfinite(fb).all()
    drift = float(np.abs(total_momentum(fa, fb) - p0).max()) / (total_mass(fa) + total_mass(fb))
    print(f"momentum drift per unit mass after 50 steps: {drift:.3e}")
    assert drift <= bound("momentum_drift_50")


# ---- mass, periodic ----------------------------------------------------------------------------------------------------------------------
SLAB_STEPS = 6000


@functools.lru_cache(maxsize=None)
def slab():
    """64 x 4 periodic: a slab of A in B between two tanh interfaces of width 2"""
    shape = (64, 4)
    x = np.arange(shape[0])[:, None] + 0.5
    profile = np.broadcast_to(0.5 * (np.tanh((x - 16.0) / 2.0) - np.tanh((x - 48.0) / 2.0)), shape)
    fa0, fb0 = at_rest(*two_sided(profile))
    bm, mm = ref.no_walls(shape, LAT)
    fa, fb = ref.run(fa0, fb0, bm, mm, [], cases.OMEGA, LAT, separating(), SLAB_STEPS, policy=POLICY)
    return fa0, fb0, fa, fb, parts_of(fa, fb, bm, mm, [], separating())


def test_both_masses_are_conserved_in_a_periodic_box():
    fa0, fb0, fa, fb, parts = slab()
    assert np.isfinite(fa).all() and np.isfinite(fb).all()
    rho_a = parts["rho_a"][0]
    assert rho_a[32, 0] > 0.9 and rho_a[0, 0] < 0.1  # still two regions
    drift = max(abs(total_mass(f) - total_mass(f0)) / total_mass(f0) for f, f0 in ((fa, fa0), (fb, fb0)))
    print(f"relative mass drift of either component after {SLAB_STEPS} steps, periodic: {drift:.3e}")
    assert drift <= bound("mass_drift_periodic")


# ---- reduction to the fluid step -----------------------------------------------------------------------------------------------------------
def test_without_interaction_the_sum_of_the_two_sets_follows_the_fluid_step():
    """all G = 0, omega_A = omega_B, f^A = f^B = f / 2: f^A + f^B follows the oracle's BGK step up to rounding (u' is formed by a division
    the plain step does not have, and each half is rounded by itself)"""
    shape = (16, 12)
    omega = 1.2
    f = cases.random_states(shape, LAT, POLICY, seed=5, lo=0.8, hi=1.2)[0]
    fa = fb = 0.5 * f
    bm, mm = ref.no_walls(shape, LAT)
    fa, fb = ref.run(fa, fb, bm, mm, [], omega, LAT, ref.Mixture(0.0), 20, policy=POLICY)
    f = orc.run(f, bm, mm, [], omega, LAT, 20, policy=POLICY)
    distance = float(np.abs((fa + fb) - f).max())
    print(f"max |f^A + f^B - f| after 20 steps: {distance:.3e}")
    assert distance <= bound("reduction_distance")


# ---- mixing threshold ------------------------------------------------------------------------------------------------------------------
MIX_MODE, MIX_STEPS = 8, 50


def perturbation_growth(g_ab, rho0=1.0, steps=MIX_STEPS):
    """a symmetric mixture rho_A = rho_B = rho0 with a sine of amplitude 1e-3 and wavelength 8 in rho_A - rho_B, 64 x 4 periodic ->
    amplitude of that Fourier mode after `steps` over its start value.  (Short, because above the threshold a mixture of total density 2
    goes on to separate completely, and rounding noise at the grid scale grows with it: at G_AB rho0 = 2 the run is finite at 150 steps
    with this wave and no longer with one of wavelength 16.)"""
    shape = (64, 4)
    x = np.arange(shape[0])[:, None]
    wave = np.broadcast_to(1e-3 * np.sin(2.0 * np.pi * MIX_MODE * x / shape[0]), shape)
    fa, fb = at_rest(rho0 + wave, rho0 - wave)
    bm, mm = ref.no_walls(shape, LAT)

    def amplitude(fa, fb):
        parts = parts_of(fa, fb, bm, mm, [], ref.Mixture(g_ab))
        return float(np.abs(np.fft.fft((parts["rho_a"][0] - parts["rho_b"][0]).mean(axis=1))[MIX_MODE]))

    a0 = amplitude(fa, fb)
    fa, fb = ref.run(fa, fb, bm, mm, [], 1.0, LAT, ref.Mixture(g_ab), steps, policy=POLICY)
    assert np.isfinite(fa).all() and np.isfinite(fb).all()
    return amplitude(fa, fb) / a0


def test_a_symmetric_mixture_mixes_below_the_threshold_and_separates_above():
    """the continuum estimate of the threshold is G_AB rho0 = 1 (linearising grad ln rho_A = -G_AB grad rho_B); only the two signs are
    asserted"""
    below, above = perturbation_growth(0.5), perturbation_growth(2.0)
    print(f"amplitude of the rho_A - rho_B mode after {MIX_STEPS} steps over its start: G_AB rho0 = 0.5: {below:.3e}, G_AB rho0 = 2: {above:.3e}")
    assert below < 1.0 < above


# ---- Laplace law ---------------------------------------------------------------------------------------------------------------------
def droplet(radius, g_ab=G_SEPARATING, steps=6000):
    shape = (64, 64)
    mix = ref.Mixture(g_ab)
    x, y = np.meshgrid(np.arange(shape[0]) + 0.5, np.arange(shape[1]) + 0.5, indexing="ij")
    r = np.sqrt((x - 32.0) ** 2 + (y - 32.0) ** 2)
    fa, fb = at_rest(*two_sided(0.5 * (1.0 - np.tanh((r - radius) / 2.0))))
    bm, mm = ref.no_walls(shape, LAT)
    fa, fb = ref.run(fa, fb, bm, mm, [], 1.0, LAT, mix, steps, policy=POLICY)
    parts = parts_of(fa, fb, bm, mm, [], mix)
    rho_a, rho_b = parts["rho_a"][0], parts["rho_b"][0]
    area = float((rho_a > 0.5 * (rho_a[32, 32] + rho_a[0, 0])).sum())
    R = np.sqrt(area / np.pi)
    dp = float(ref.pressure(mix, rho_a[32, 32], rho_b[32, 32]) - ref.pressure(mix, rho_a[0, 0], rho_b[0, 0]))
    return dp * R, R, dp, float(np.sqrt((parts["u_phys"] ** 2).sum(axis=0)).max())


@pytest.mark.slow
def test_laplace_law_pressure_jump_times_radius_is_constant():
    """(p_in - p_out) R for droplets of A in B of initial radius 10, 14 and 18; R from the area above the mid density of A"""
    sigma = []
    for radius in (10, 14, 18):
        s, R, dp, umax = droplet(radius)
        print(f"initial radius {radius}: R = {R:.3f}, p_in - p_out = {dp:.5e}, product {s:.5f}, max |u| = {umax:.3e}")
        sigma.append(s)
    spread = (max(sigma) - min(sigma)) / np.mean(sigma)
    print(f"relative spread of (p_in - p_out) R: {spread:.3e}")
    assert min(sigma) > 0.05
    assert spread <= bound("laplace_spread")


# ---- wetting (and the walled mass pin) ---------------------------------------------------------------------------------------------------
WET_STEPS = 3000
WALL_PAIRS = {"A-wetting": (0.65, 0.35), "neutral": (0.5, 0.5), "B-wetting": (0.35, 0.65)}


@functools.lru_cache(maxsize=None)
def sessile_droplet(wetting):
    """80 x 32, resting halfway walls at both y faces (hand-corrected plate bits), x periodic; half a droplet of A of radius 14 on the
    bottom wall -> (base width, height, larger mass drift of the two components)"""
    shape = (80, 32)
    mix = separating()
    setup = cases.halfway_plates(shape, WALL_PAIRS[wetting], WALL_PAIRS[wetting])
    bcs, wall_density = setup.oracle()
    bm, mm = setup.masks(shape, LAT, bcs)
    x, y = np.meshgrid(np.arange(shape[0]) + 0.5, np.arange(shape[1]), indexing="ij")
    r = np.sqrt((x - 40.0) ** 2 + y**2)
    fa0, fb0 = at_rest(*two_sided(0.5 * (1.0 - np.tanh((r - 14.0) / 2.0))))
    fa, fb = ref.run(fa0, fb0, bm, mm, bcs, 1.0, LAT, mix, WET_STEPS, wall_density=wall_density, policy=POLICY)
    assert np.isfinite(fa).all() and np.isfinite(fb).all()
    rho_a = parts_of(fa, fb, bm, mm, bcs, mix, wall_density)["rho_a"][0]
    mid = 0.5 * (RHO_MAJOR + RHO_MINOR)
    base, height = int((rho_a[:, 0] > mid).sum()), int((rho_a[40, :] > mid).sum())
    drift = max(abs(total_mass(f) - total_mass(f0)) / total_mass(f0) for f, f0 in ((fa, fa0), (fb, fb0)))
    return base, height, drift


def test_base_width_of_a_sessile_droplet_follows_the_wall_densities():
    shapes = {w: sessile_droplet(w)[:2] for w in WALL_PAIRS}
    print("wall densities -> (base width, height):", shapes)
    assert shapes["A-wetting"][0] > shapes["neutral"][0] > shapes["B-wetting"][0] > 0


def test_both_masses_are_conserved_between_resting_halfway_walls():
    drift = sessile_droplet("neutral")[2]
    print(f"relative mass drift of either component after {WET_STEPS} steps, walled: {drift:.3e}")
    assert drift <= bound("mass_drift_walled")


# ---- viscosity contrast: measured, not asserted ---------------------------------------------------------------------------------------------
def layered_poiseuille(n, g=1e-6, nu_a=1.0 / 6.0, nu_b=1.0 / 24.0):
    """A (viscosity 1/6, omega 1) below B (viscosity 1/24, omega 1.6) between resting halfway plates n cells apart, 4 cells periodic along
    the flow, driven by force_vector; each plate carries the densities of the layer it touches (a wall like the fluid at it: no net force
    there).  12 n^2 steps, two diffusion times (n / 2)^2 / nu of the slower layer -> (relative L2 distance of the barycentric velocity from
    the sharp-interface profile of two layers with the measured mean total densities, the same over the rows more than 4 cells from the
    interface, the smallest density, the component and the row where it sits, the steps)."""
    shape = (4, n)
    omega = (1.0 / (3.0 * nu_a + 0.5), 1.0 / (3.0 * nu_b + 0.5))
    mix = separating()
    setup = cases.halfway_plates(shape, (RHO_MAJOR, RHO_MINOR), (RHO_MINOR, RHO_MAJOR))
    bcs, wall_density = setup.oracle()
    bm, mm = setup.masks(shape, LAT, bcs)
    y = np.arange(n)[None, :] + 0.5
    fa, fb = at_rest(*two_sided(np.broadcast_to(0.5 * (1.0 - np.tanh((y - 0.5 * n) / 2.0)), shape)))
    kw = dict(wall_density=wall_density, policy=POLICY, force_vector=np.array([g, 0.0]))
    steps = 12 * n * n
    for _ in range(steps):
        fa, fb = ref.step(fa, fb, bm, mm, bcs, omega, LAT, mix, **kw)
    parts = {}
    ref.step(fa, fb, bm, mm, bcs, omega, LAT, mix, parts=parts, **kw)
    rows = {name: parts[key][0].mean(axis=0) for name, key in (("A", "rho_a"), ("B", "rho_b"))}
    which = min(rows, key=lambda name: rows[name].min())
    u = parts["u_phys"][0].mean(axis=0)
    rho = rows["A"] + rows["B"]
    # sharp interface at h = n / 2, walls at 0 and n: mu u'' = -rho g in each layer, u and mu u' continuous at h
    h, H = 0.5 * n, float(n)
    rho_lo, rho_hi = rho[: n // 2].mean(), rho[n // 2 :].mean()
    mu_a, mu_b, ga, gb = nu_a * rho_lo, nu_b * rho_hi, rho_lo * g, rho_hi * g
    # u_a = -ga y^2 / (2 mu_a) + p y,  u_b = -gb (y - H)^2 / (2 mu_b) + q (y - H)
    A = np.array([[h, -(h - H)], [mu_a, -mu_b]])
    b = np.array([ga * h * h / (2 * mu_a) - gb * (h - H) ** 2 / (2 * mu_b), ga * h - gb * (h - H)])
    p, q = np.linalg.solve(A, b)
    yy = np.arange(n) + 0.5
    exact = np.where(yy < h, -ga * yy**2 / (2 * mu_a) + p * yy, -gb * (yy - H) ** 2 / (2 * mu_b) + q * (yy - H))
    l2 = lambda keep: float(np.sqrt(((u - exact)[keep] ** 2).sum() / (exact[keep] ** 2).sum()))  # noqa: E731
    return l2(slice(None)), l2(np.abs(yy - h) > 4.0), float(rows[which].min()), which, int(rows[which].argmin()), steps


@pytest.mark.slow
def test_layered_poiseuille_flow_with_a_viscosity_contrast_is_measured():
    """Measured, NOT asserted beyond finiteness, at 32 cells across (64 takes a minute: call layered_poiseuille(64)).  The restatement
    gives 14.2 % at 32 and 16.5 % at 64 in relative L2: the distance from the sharp-interface profile does not shrink with the
    resolution, and a minority density is slightly negative (-0.032 at both).  profiles/multicomponent.md has the figures and what is and
    is not known about the cause."""
    distance, away, lowest, which, row, steps = layered_poiseuille(32)
    print(f"32 cells across, {steps} steps: relative L2 distance from the sharp-interface profile {distance:.3e} ({away:.3e} over the rows more than 4 cells "
          f"from the interface), smallest density {lowest:.3e} (component {which}, row {row})")
    assert np.isfinite(distance)


# ---- the package's mixture is the restatement's ---------------------------------------------------------------------------------------------
def test_the_packages_mixture_has_the_restatements_pressure():
    from xlb_amd.operator.stepper import ShanChenMixture

    a, b = np.linspace(0.01, 1.5, 50), np.linspace(1.2, 0.02, 50)
    mine, theirs = ref.Mixture(cases.G_AB, cases.G_AA, cases.G_BB), ShanChenMixture(G_AB=cases.G_AB, G_AA=cases.G_AA, G_BB=cases.G_BB)
    assert np.array_equal(ref.pressure(mine, a, b), theirs.pressure(a, b))
