"""The set-ups, the model and the start states shared by the multicomponent tests (host emulation, device, physics pins).  The walled
set-ups are those of tests/_multiphase_cases.py with every halfway wall at rest (the stepper refuses a wall velocity) and a PAIR of wall
densities (rho_w of A, rho_w of B) where that file has one.  TEST INFRASTRUCTURE ONLY."""

import numpy as np

from oracle import xlb_numpy as orc

import _multicomponent_ref as ref
import _multiphase_cases as mp_cases
from _multiphase_cases import Setup, Wall, block_cells, box_faces, fullway_box, halfway_plates, long_walls, periodic, solid_block  # noqa: F401

# Unequal relaxation rates and three non-zero, distinct interaction strengths: swapping S^A and S^B in F^A, or dropping omega from the
# weights of u', changes the result of every case
OMEGA = (1.2, 0.8)
G_AA, G_AB, G_BB = -0.3, 0.9, 0.2
# start state: densities of either component in [LO, HI]; the two pairs of wall densities
LO, HI = 0.4, 1.1
WALL_LO, WALL_HI = (0.9, 0.2), (0.15, 1.0)
FORCE = np.array([1e-4, -2e-4, 3e-4])


def mixture():
    return ref.Mixture(G_AB, G_AA, G_BB)


def halfway_box(shape, rho_lo, rho_hi):
    """closed by resting halfway walls: two wall-density pairs on the two faces of the last axis, none on the side walls"""
    low, high, sides = box_faces(shape)
    H = orc.KIND_HALFWAY_BB
    return Setup([Wall(H, low, rho_lo), Wall(H, high, rho_hi), Wall(H, sides)])


def random_states(shape, lat, policy, seed, lo=LO, hi=HI):
    """(f^A, f^B): two independent random equilibria in the store dtype"""
    return (mp_cases.random_state(shape, lat, policy, lo, hi, seed=seed), mp_cases.random_state(shape, lat, policy, lo, hi, seed=seed + 1000))


def force_vector(lat):
    return FORCE[: lat.d]
