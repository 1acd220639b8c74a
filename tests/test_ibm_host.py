"""CPU-side checks of the immersed-boundary stepper: the drop-in boundary (class, C ABI, ctypes), the NumPy restatement the GPU is
compared with (tests/_ibm_ref.py) pinned by properties that follow from theory, and the Voronoi-area helper."""

import ctypes
import os
import re

import numpy as np

from oracle import xlb_numpy as orc

import _ibm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IBM_SYMBOLS = ["xlbhip_ibm_create", "xlbhip_ibm_destroy", "xlbhip_ibm_set_markers", "xlbhip_ibm_step", "xlbhip_ibm_run", "xlbhip_ibm_forces",
               "xlbhip_ibm_iterations", "xlbhip_ibm_footprint"]


def test_ibm_stepper_is_importable():
    from xlb_amd.operator.stepper import IBMStepper, IncompressibleNavierStokesStepper

    assert issubclass(IBMStepper, IncompressibleNavierStokesStepper)


def test_ibm_symbols_are_declared_exported_and_bound():
    from xlb_amd import _lib

    text = open(os.path.join(ROOT, "include", "xlbhip.h")).read()
    assert "ibm_stepper.py" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in IBM_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} not declared in include/xlbhip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES


def test_helpers_are_importable():
    from xlb_amd.helper import calculate_voronoi_areas, create_ibm_fields  # noqa: F401


# ---- the restatement, pinned from theory ---------------------------------------------------------------------------------------
def test_weights_of_a_marker_sum_to_one_away_from_the_faces():
    """Peskin's function satisfies sum_i phi(x - i) = 1 for every x, so the product weights of a full support sum to 1; a support
    clipped by a face sums to less."""
    rng = np.random.default_rng(3)
    shape = (12, 10, 14)
    for X in rng.uniform(2.0, 8.0, size=(50, 3)):
        _, w = ref.support(X, shape, np.float64)
        assert abs(w.sum() - 1.0) <= 4e-15
    for X in ([0.7, 5.0, 5.0], [5.0, 9.6, 5.0], [5.0, 5.0, 12.9]):
        _, w = ref.support(X, shape, np.float64)
        assert 0.0 < w.sum() < 1.0 - 1e-3


def _case(policy, n_markers=60, shape=(14, 12, 12), seed=1):
    lat = orc.Lattice("D3Q19")
    f = orc.perturbed_init(shape, lat, policy, seed=seed)
    pos = ref.fibonacci_sphere(n_markers, 3.3, (6.7, 6.1, 5.6))
    areas = np.full(n_markers, 4 * np.pi * 3.3**2 / n_markers, dtype=np.float32)
    vel = np.tile(np.array([0.02, 0.01, -0.005], dtype=np.float32), (n_markers, 1))
    return lat, f, pos, areas, vel


def test_correction_keeps_the_mass_and_shifts_the_velocity_by_g():
    """feq(rho, u + G) - feq(rho, u) has zeroth moment 0 and first moment rho G."""
    lat, f, pos, areas, vel = _case("FP64FP64")
    out = ref.couple(f, pos, areas, vel, lat, "FP64FP64", max_iterations=3, tolerance=0.0, relaxation=0.5)
    rho0, u0 = orc.macroscopic(f, lat)
    rho1, u1 = orc.macroscopic(out["f"], lat)
    assert np.abs(rho1 - rho0).max() <= 1e-14
    assert np.abs((u1 - u0) - out["G"]).max() <= 1e-14
    assert np.abs(out["G"]).max() > 1e-3  # the body does something
    assert np.array_equal(out["f"][:, out["W"] == 0], f[:, out["W"] == 0])  # nothing outside the footprint


def test_result_does_not_depend_on_the_order_of_the_markers():
    lat, f, pos, areas, vel = _case("FP64FP64")
    vel = vel * np.linspace(0.5, 1.5, len(pos), dtype=np.float32)[:, None]
    a = ref.couple(f, pos, areas, vel, lat, "FP64FP64", relaxation=0.5)
    p = np.random.default_rng(0).permutation(len(pos))
    b = ref.couple(f, pos[p], areas[p], vel[p], lat, "FP64FP64", relaxation=0.5)
    assert np.abs(a["f"] - b["f"]).max() <= 1e-15
    assert np.abs(a["forces"][p] - b["forces"]).max() <= 1e-15


def test_early_exit_of_the_sweep_loop():
    """tolerance 0 never computes a residual: every sweep runs.  A tolerance above every |U - u_k| keeps the flag down in the second
    sweep (the first that computes one), so the third does not run."""
    lat, f, pos, areas, vel = _case("FP32FP32")
    assert ref.couple(f, pos, areas, vel, lat, "FP32FP32", max_iterations=6, tolerance=0.0)["sweeps"] == 6
    assert ref.couple(f, pos, areas, vel, lat, "FP32FP32", max_iterations=6, tolerance=1.0)["sweeps"] == 2
    assert ref.couple(f, pos, areas, vel, lat, "FP32FP32", max_iterations=4, tolerance=1e-5)["sweeps"] == 4
    assert ref.couple(f, pos, areas, vel, lat, "FP32FP32", max_iterations=1, tolerance=1.0)["sweeps"] == 1


# ---- helper --------------------------------------------------------------------------------------------------------------------
def test_voronoi_areas_of_an_icosphere_sum_to_its_surface_area():
    from xlb_amd.helper.ibm_helper import calculate_voronoi_areas, icosphere

    verts, faces = icosphere(3)
    verts = verts * 7.5 + np.array([20.0, 11.0, 12.5])
    areas = calculate_voronoi_areas(verts, faces)
    tri = verts[faces]
    surface = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    assert areas.dtype == np.float32 and areas.shape == (len(verts),) and (areas > 0).all()
    assert abs(areas.sum(dtype=np.float64) - surface) <= 1e-6 * surface
    assert abs(surface - 4 * np.pi * 7.5**2) <= 0.01 * surface  # (and the polyhedron is close to the sphere)
    # a single right triangle: the right-angle corner has cotangent 0, so it gets A (cot_beta + cot_gamma) / 2 = A / 2
    a = calculate_voronoi_areas(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=float), np.array([[0, 1, 2]]))
    assert np.allclose(a, [0.25, 0.125, 0.125])
