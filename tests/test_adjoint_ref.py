"""Pins the adjoint restatement tests/_adjoint_ref.py to the ORACLE's forward step: central finite differences of orc.run against the
adjoint chain (second-order convergence is the acceptance, not a tolerance), the omega derivative the same way, and the dot-product
identity <J v, w> = <v, J^T w> with the forward-mode twin, to rounding."""

import math

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _adjoint_cases as cases
import _adjoint_ref as ref

POLICY, OMEGA, STEPS = "FP64FP64", 1.3, 3


def setup(name):
    lat, shape, bcs = cases.HOST_CASES[name]()
    bm, mm = cases.masks(shape, lat, bcs)
    f_0 = orc.perturbed_init(shape, lat, POLICY, seed=11, amp_rho=0.02, amp_u=0.03)
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, f_0.shape)
    w = rng.uniform(-1, 1, f_0.shape)
    return lat, shape, bcs, bm, mm, f_0, v, w


def run(f, bm, mm, bcs, lat, omega=OMEGA):
    return orc.run(f, bm, mm, bcs, omega, lat, STEPS, POLICY)


def adjoint_chain(f_0, w, bm, mm, bcs, lat):
    states, _ = ref.forward_states(f_0, bm, mm, bcs, OMEGA, lat, STEPS, POLICY)
    return ref.backward(states, w, bm, mm, bcs, OMEGA, lat, POLICY)


def tangent_chain(f_0, v, bm, mm, bcs, lat, **kw):
    states, _ = ref.forward_states(f_0, bm, mm, bcs, OMEGA, lat, STEPS, POLICY)
    for f_n in states:
        v = ref.tangent_step(f_n, v, bm, mm, bcs, OMEGA, lat, POLICY, **kw)
    return v


def check_order(gaps, label):
    """gaps at h = 1e-3, 1e-4[, 1e-5]: a factor 50 .. 200 per decade (measured: 100), and still falling at 1e-5"""
    print(label, " ".join(f"{g:.3e}" for g in gaps))
    assert 50.0 < gaps[0] / gaps[1] < 200.0, f"{label}: gap {gaps[0]:.3e} -> {gaps[1]:.3e} is not second order"
    if len(gaps) > 2:
        assert gaps[2] < gaps[1], f"{label}: gap grows from h = 1e-4 ({gaps[1]:.3e}) to 1e-5 ({gaps[2]:.3e})"


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_adjoint_converges_to_finite_differences_of_the_oracle(name):
    lat, shape, bcs, bm, mm, f_0, v, w = setup(name)
    lam_0, _ = adjoint_chain(f_0, w, bm, mm, bcs, lat)
    adj = float(np.sum(v * lam_0))
    gaps = []
    for h in (1e-3, 1e-4, 1e-5):
        fd = float(np.sum((run(f_0 + h * v, bm, mm, bcs, lat) - run(f_0 - h * v, bm, mm, bcs, lat)) * w)) / (2 * h)
        gaps.append(abs(fd - adj) / abs(adj))
    check_order(gaps, f"{name} <dS v, w> vs <v, J^T w>:")


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_tangent_converges_to_finite_differences_of_the_oracle(name):
    lat, shape, bcs, bm, mm, f_0, v, w = setup(name)
    jv = tangent_chain(f_0, v, bm, mm, bcs, lat)
    gaps = []
    for h in (1e-3, 1e-4, 1e-5):
        fd = (run(f_0 + h * v, bm, mm, bcs, lat) - run(f_0 - h * v, bm, mm, bcs, lat)) / (2 * h)
        gaps.append(float(np.linalg.norm(fd - jv) / np.linalg.norm(jv)))
    check_order(gaps, f"{name} tangent:")


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_omega_derivative_converges_to_finite_differences_of_the_oracle(name):
    lat, shape, bcs, bm, mm, f_0, v, w = setup(name)
    _, terms = adjoint_chain(f_0, w, bm, mm, bcs, lat)
    adj = math.fsum(float(t) for step in terms for t in step.ravel())
    gaps = []
    for h in (1e-3, 1e-4):
        fd = float(np.sum((run(f_0, bm, mm, bcs, lat, OMEGA + h) - run(f_0, bm, mm, bcs, lat, OMEGA - h)) * w)) / (2 * h)
        gaps.append(abs(fd - adj) / abs(adj))
    check_order(gaps, f"{name} dL/domega:")


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_dot_product_identity_to_rounding(name):
    """<J v, w> and <v, J^T w> add up the same products in two orders: they agree within q N_cells n_steps 2^-52 sum|products|, the sum
    of absolute products bounded from above by the chain run on absolute values."""
    lat, shape, bcs, bm, mm, f_0, v, w = setup(name)
    lam_0, _ = adjoint_chain(f_0, w, bm, mm, bcs, lat)
    lhs = float(np.sum(tangent_chain(f_0, v, bm, mm, bcs, lat) * w))
    rhs = float(np.sum(v * lam_0))
    products = float(np.sum(tangent_chain(f_0, v, bm, mm, bcs, lat, absolute=True) * np.abs(w)))
    bound = lat.q * int(np.prod(shape)) * STEPS * 2.0**-52 * products
    print(f"{name}: <Jv,w> = {lhs:.17g}, <v,JTw> = {rhs:.17g}, |difference| = {abs(lhs - rhs):.3e}, bound = {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_omega_term_of_one_step_is_the_contraction_with_the_omega_tangent():
    lat, shape, bcs, bm, mm, f_0, v, w = setup("cavity3d-fullway-D3Q19")
    _, terms = ref.adjoint_step(f_0, w, bm, mm, bcs, OMEGA, lat, POLICY)
    direct = np.sum(ref.omega_tangent(f_0, bm, mm, bcs, OMEGA, lat, POLICY) * w, axis=0)
    assert np.allclose(terms, direct, rtol=0, atol=1e-15 * lat.q)


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP32"])
def test_narrow_policies_stay_close_to_fp64(policy):
    """the same rules in fp32 compute or fp32 storage: a coarse check that the dtype plumbing does not change the mathematics.  Bound:
    a lam value is a sum of at most q + 3 d + 3 = 18 products of size <= 3 (|lam| <= 1, coefficients of order one), each rounded to
    2^-24, on inputs rounded to 2^-24 themselves: 2 x 18 x 3 x 6e-8 = 6.5e-6 < 1e-5."""
    lat, shape, bcs, bm, mm, f_0, v, w = setup("cavity2d-halfway-D2Q9")
    S = orc.store_dtype(policy)
    lam64, _ = ref.adjoint_step(f_0, w, bm, mm, bcs, OMEGA, lat, "FP64FP64")
    lam, terms = ref.adjoint_step(f_0.astype(S), w.astype(S), bm, mm, bcs, OMEGA, lat, policy)
    assert lam.dtype == S and terms.dtype == orc.compute_dtype(policy)
    assert np.abs(lam - lam64).max() < 1e-5
