"""Physics pins of the NumPy restatement of the Shan-Chen step (tests/_multiphase_ref.py): what the scheme must do whatever code runs it.
FP64FP64 on D2Q9, omega = 1.  Every bound is twice the figure measured with the committed restatement (MEASURED below, recorded in
profiles/multiphase.md); each test prints its figure before it asserts."""

import functools
import math

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _multiphase_cases as cases
import _multiphase_ref as ref

POLICY = "FP64FP64"
LAT = orc.Lattice("D2Q9")
OMEGA = 1.0
G_EXP = -5.5

# the figures of the committed restatement; asserted at twice each
MEASURED = {
    "force_sum": 4.441e-16,  # max |sum_x F_a| over four random fields, max |F| = 0.267
    "momentum_drift_50": 2.029e-17,  # |P(50) - P(0)| / mass, exact sums
    "mass_drift_periodic": 5.391e-13,  # relative, 6000 steps, the flat interface
    "mass_drift_walled": 3.937e-13,  # relative, 4000 steps, the sessile droplet at wall density 1.2
    "flat_pressure_difference": 3.390e-08,  # |p(liquid) - p(vapour)|, densities 0.30645 and 0.01854 (ratio 16.5)
    "flat_max_velocity": 6.770e-07,  # max |u_bare + F / (2 rho)|
    "laplace_spread": 1.194e-02,  # (max - min) / mean of (p_in - p_out) R = 0.09404, 0.09484, 0.09517
}


def bound(key):
    return 2.0 * MEASURED[key]


def total_mass(f):
    """exactly rounded, so that a drift is the scheme's and not the sum's"""
    return math.fsum(f.astype(np.float64).ravel())


def total_momentum(f):
    f = f.astype(np.float64)
    return np.array([math.fsum((LAT.c[a][(slice(None),) + (None,) * LAT.d] * f).ravel()) for a in range(LAT.d)])


def parts_of(f, bm, mm, bcs, model, wall_density=None):
    return ref.outputs(f, bm, mm, bcs, LAT, model, wall_density, POLICY)


# ---- momentum ------------------------------------------------------------------------------------------------------------------------
def random_rest_state(seed):
    shape = (16, 12)
    rho = np.random.default_rng(seed).uniform(0.1, 2.5, shape)
    return shape, ref.init_at_rest(rho, LAT, POLICY)


def test_the_interaction_force_sums_to_zero_in_a_periodic_box():
    model = ref.Exponential(G_EXP)
    worst, largest = 0.0, 0.0
    for seed in range(4):
        shape, f = random_rest_state(seed)
        bm, mm = ref.no_walls(shape, LAT)
        F = parts_of(f, bm, mm, [], model)["force"]
        worst = max(worst, float(np.abs(F.reshape(LAT.d, -1).sum(axis=1)).max()))
        largest = max(largest, float(np.abs(F).max()))
    print(f"max |sum_x F| = {worst:.3e} with max |F| = {largest:.3e}")
    assert largest > 0.1
    assert worst <= bound("force_sum")


def test_total_momentum_stays_put_over_fifty_steps():
    model = ref.Exponential(G_EXP)
    shape, f = random_rest_state(0)
    bm, mm = ref.no_walls(shape, LAT)
    p0 = total_momentum(f)
    f = ref.run(f, bm, mm, [], OMEGA, LAT, model, 50, policy=POLICY)
    assert np.isfinite(f).all()
    drift = float(np.abs(total_momentum(f) - p0).max()) / total_mass(f)
    print(f"momentum drift per unit mass after 50 steps: {drift:.3e}")
    assert drift <= bound("momentum_drift_50")


# ---- flat interface (and the periodic mass pin) ------------------------------------------------------------------------------------------
FLAT_STEPS = 6000


@functools.lru_cache(maxsize=None)
def flat_interface():
    """Carnahan-Starling at 0.8 Tc, 64 x 4 periodic: a liquid slab between two tanh interfaces of width 2.5"""
    shape = (64, 4)
    model = ref.CarnahanStarling(0.8 * ref.CarnahanStarling.critical_temperature())
    x = np.arange(shape[0])[:, None] + 0.5
    profile = 0.02 + 0.5 * (0.31 - 0.02) * (np.tanh((x - 16.0) / 2.5) - np.tanh((x - 48.0) / 2.5))
    f0 = ref.init_at_rest(np.broadcast_to(profile, shape), LAT, POLICY)
    bm, mm = ref.no_walls(shape, LAT)
    f = ref.run(f0, bm, mm, [], OMEGA, LAT, model, FLAT_STEPS, policy=POLICY)
    return model, f0, f, parts_of(f, bm, mm, [], model)


def test_flat_interface_coexistence_pressures_agree_and_the_fluid_rests():
    model, _, f, parts = flat_interface()
    rho = parts["rho"][0]
    liquid, vapour = float(rho[32, 0]), float(rho[0, 0])
    dp = abs(float(ref.pressure(model, liquid)) - float(ref.pressure(model, vapour)))
    umax = float(np.abs(parts["u_phys"]).max())
    print(f"liquid {liquid:.5f} vapour {vapour:.5f} ratio {liquid / vapour:.2f}  |p_l - p_v| = {dp:.3e}  max |u| = {umax:.3e}")
    assert 0.28 < liquid < 0.33 and 0.015 < vapour < 0.025  # two phases, near the Maxwell densities of 0.8 Tc
    assert dp <= bound("flat_pressure_difference")
    assert umax <= bound("flat_max_velocity")


def test_mass_is_conserved_in_a_periodic_box():
    _, f0, f, _ = flat_interface()
    drift = abs(total_mass(f) - total_mass(f0)) / total_mass(f0)
    print(f"relative mass drift after {FLAT_STEPS} steps, periodic: {drift:.3e}")
    assert drift <= bound("mass_drift_periodic")


# ---- Laplace law ---------------------------------------------------------------------------------------------------------------------
def droplet(radius, steps=6000):
    shape = (64, 64)
    model = ref.Exponential(G_EXP)
    x, y = np.meshgrid(np.arange(shape[0]) + 0.5, np.arange(shape[1]) + 0.5, indexing="ij")
    r = np.sqrt((x - 32.0) ** 2 + (y - 32.0) ** 2)
    rho0 = 0.12 + 0.5 * (2.0 - 0.12) * (1.0 - np.tanh((r - radius) / 2.0))
    bm, mm = ref.no_walls(shape, LAT)
    f = ref.run(ref.init_at_rest(rho0, LAT, POLICY), bm, mm, [], OMEGA, LAT, model, steps, policy=POLICY)
    rho = parts_of(f, bm, mm, [], model)["rho"][0]
    inside, outside = float(rho[32, 32]), float(rho[0, 0])
    area = float((rho > 0.5 * (inside + outside)).sum())
    R = np.sqrt(area / np.pi)
    dp = float(ref.pressure(model, inside) - ref.pressure(model, outside))
    return dp * R, R, dp


@pytest.mark.slow
def test_laplace_law_pressure_jump_times_radius_is_constant():
    """(p_in - p_out) R for droplets of initial radius 10, 14 and 18; R from the area above the mid density"""
    sigma = []
    for radius in (10, 14, 18):
        s, R, dp = droplet(radius)
        print(f"initial radius {radius}: R = {R:.3f}, p_in - p_out = {dp:.5e}, product {s:.5f}")
        sigma.append(s)
    spread = (max(sigma) - min(sigma)) / np.mean(sigma)
    print(f"relative spread of (p_in - p_out) R: {spread:.3e}")
    assert min(sigma) > 0.05
    assert spread <= bound("laplace_spread")


# ---- wetting (and the walled mass pin) ---------------------------------------------------------------------------------------------------
WET_STEPS = 4000


@functools.lru_cache(maxsize=None)
def sessile_droplet(rho_w):
    """96 x 40, halfway walls at both y faces, x periodic; half a droplet of radius 16 on the bottom wall -> (base width, height, mass drift)"""
    shape = (96, 40)
    model = ref.Exponential(G_EXP)
    setup = cases.halfway_plates(shape, rho_w, rho_w)
    bcs, wall_density = setup.oracle()
    bm, mm = setup.masks(shape, LAT, bcs)
    x, y = np.meshgrid(np.arange(shape[0]) + 0.5, np.arange(shape[1]), indexing="ij")
    r = np.sqrt((x - 48.0) ** 2 + y**2)
    rho0 = 0.105 + 0.5 * (2.3 - 0.105) * (1.0 - np.tanh((r - 16.0) / 2.0))
    f0 = ref.init_at_rest(rho0, LAT, POLICY)
    f = ref.run(f0, bm, mm, bcs, OMEGA, LAT, model, WET_STEPS, wall_density=wall_density, policy=POLICY)
    rho = parts_of(f, bm, mm, bcs, model, wall_density)["rho"][0]
    assert np.isfinite(rho).all()
    base = int((rho[:, 0] > 1.2).sum())
    height = int((rho[48, :] > 1.2).sum())
    return base, height, abs(total_mass(f) - total_mass(f0)) / total_mass(f0)


def test_base_width_of_a_sessile_droplet_rises_with_the_wall_density():
    shapes = {rho_w: sessile_droplet(rho_w)[:2] for rho_w in (0.8, 1.2, 1.8)}
    print("wall density -> (base width, height):", shapes)
    assert 0 < shapes[0.8][0] < shapes[1.2][0] < shapes[1.8][0]
    assert shapes[0.8][1] > shapes[1.2][1] > shapes[1.8][1] > 0


def test_mass_is_conserved_between_halfway_walls():
    drift = sessile_droplet(1.2)[2]
    print(f"relative mass drift after {WET_STEPS} steps, walled: {drift:.3e}")
    assert drift <= bound("mass_drift_walled")


# ---- the package's pseudopotential classes are the restatement's -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_packages_pseudopotentials_evaluate_like_the_restatements(dtype):
    from xlb_amd.operator.stepper import CarnahanStarling, ShanChenDensity, ShanChenExponential

    rho = np.linspace(0.0, 0.36, 500).astype(dtype)
    t_cs = 0.8 * ref.CarnahanStarling.critical_temperature()
    assert CarnahanStarling(t_cs).critical_temperature == ref.CarnahanStarling.critical_temperature()
    for mine, theirs in ((ref.CarnahanStarling(t_cs), CarnahanStarling(t_cs)), (ref.Density(-0.6), ShanChenDensity(-0.6)),
                         (ref.Exponential(G_EXP, 1.5), ShanChenExponential(G_EXP, 1.5))):
        a, b = mine.psi(rho), theirs.psi(rho)
        assert a.dtype == b.dtype == np.dtype(dtype) and np.array_equal(a, b)
        assert np.array_equal(ref.pressure(mine, rho), theirs.pressure(rho))
