"""Host side of the rigid bodies of IBMStepper: RigidMotion's poses, the validation of set_bodies (helper.ibm_helper.declare_bodies, which
needs no device) and the NumPy restatement of the move and the loads
(tests/_ibm_motion_ref.py) against a plain fp64 rigid transform."""

import numpy as np
import pytest

from xlb_amd.helper.ibm_helper import IBMBody, RigidMotion, declare_bodies

import _ibm_motion_ref as mref
import _ibm_ref as ref

MOTION = dict(centre=(9.0, 10.0, 11.85), axis=(0, 0, 1), rate=0.008, velocity=(0.02, 0.01, -0.005))


def rodrigues(axis, angle):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * np.outer(k, k)


@pytest.mark.parametrize("axis", [(0, 0, 1), (1, -2, 0.5), (0, 3, 0)])
def test_rigid_motion_poses(axis):
    m = RigidMotion(centre=(9.0, 10.0, 11.85), axis=axis, rate=0.008, velocity=(0.02, 0.01, -0.005), phase=0.3)
    unit = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    for t in (0, 1, 7, 11, 100000):
        R, c, w, v = m.at(t)
        assert all(a.dtype == np.float64 for a in (R, c, w, v)) and R.shape == (3, 3) and c.shape == w.shape == v.shape == (3,)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
        # the TOTAL angle, evaluated once: equal to a direct Rodrigues evaluation at phase + rate t (a product of t per-step
        # rotations would be off by about t roundings)
        assert np.abs(R - rodrigues(axis, 0.3 + 0.008 * t)).max() <= 4e-16
        assert np.array_equal(c, np.array([9.0, 10.0, 11.85]) + np.array([0.02, 0.01, -0.005]) * float(t))
        assert np.array_equal(w, 0.008 * unit) and np.array_equal(v, [0.02, 0.01, -0.005])
        assert np.abs(R @ unit - unit).max() <= 1e-15  # the axis is fixed
    assert np.array_equal(RigidMotion((0, 0, 0), axis, 0.5).at(0)[0], np.eye(3))  # angle 0
    assert np.array_equal(RigidMotion((0, 0, 0), axis, 0.0, phase=0.0).at(12)[0], np.eye(3))


def test_rigid_motion_does_not_accumulate():
    m = RigidMotion(**MOTION)
    product = np.eye(3)
    step = m.at(1)[0]
    for _ in range(5000):
        product = step @ product
    exact = rodrigues((0, 0, 1), 0.008 * 5000)
    assert np.abs(m.at(5000)[0] - exact).max() <= 4e-16
    assert np.array_equal(m.at(5000)[0], RigidMotion(**MOTION).at(5000)[0])
    assert np.abs(product - exact).max() > np.abs(m.at(5000)[0] - exact).max()


def test_zero_axis_is_refused():
    with pytest.raises(ValueError, match="axis"):
        RigidMotion((0, 0, 0), (0, 0, 0), 0.1)


def test_set_bodies_validation_names_the_body():
    def declare(bodies):
        return declare_bodies(bodies, 400, lambda: pytest.fail("no resting body needs the uploaded positions here"))

    with pytest.raises(ValueError, match=r"body 1.*300:401.*out of bounds.*400"):
        declare([IBMBody(slice(0, 100)), IBMBody(slice(300, 401))])
    with pytest.raises(ValueError, match=r"body 0.*out of bounds"):
        declare([IBMBody(slice(-5, 100))])
    with pytest.raises(ValueError, match=r"body 0.*out of bounds"):
        declare([IBMBody(slice(200, 100))])
    with pytest.raises(ValueError, match=r"bodies 0 and 2 overlap"):
        declare([IBMBody(slice(0, 100)), IBMBody(slice(200, 300)), IBMBody(slice(99, 150))])
    with pytest.raises(ValueError, match=r"body 0.*contiguous"):
        declare([IBMBody(slice(0, 100, 2))])
    with pytest.raises(ValueError, match=r"65 bodies.*64"):
        declare([IBMBody(slice(i, i + 1)) for i in range(65)])
    with pytest.raises(TypeError):
        IBMBody(markers=[0, 1, 2])
    with pytest.raises(TypeError):
        IBMBody(slice(0, 3), motion="spin")


def test_restatement_is_a_rigid_transform():
    X0 = ref.fibonacci_sphere(400, 5.3, (11.3, 12.6, 11.85))
    m = RigidMotion(**MOTION)
    c0 = m.at(0)[1]
    for t in (0, 5, 11):
        R, c, w, v = mref.pose(m, t)
        X, U = mref.move(X0, c0, R, c, w, v)
        assert X.dtype == U.dtype == np.float32
        exact = c + (X0.astype(np.float64) - c0) @ R.T
        # fp64 rounding of three products and three sums of magnitude <= 20, then ONE float32 rounding
        assert np.abs(X.astype(np.float64) - exact).max() <= 2.0**-24 * 32
        Ue = v + np.cross(w, X.astype(np.float64) - c)
        assert np.abs(U.astype(np.float64) - Ue).max() <= 2.0**-24 * 0.125  # |U| < 0.125: one float32 rounding of at most 2^-28, fp64 roundings far below
        # rigid: distances to the centre are kept
        d0 = np.linalg.norm(X0.astype(np.float64) - c0, axis=1)
        assert np.abs(np.linalg.norm(X.astype(np.float64) - c, axis=1) - d0).max() <= 4e-6
    assert np.array_equal(mref.move(X0, c0, *mref.pose(m, 0))[0], X0)  # identity at t = 0: the uploaded positions, bit for bit
    # the inputs the GPU tests rely on: nothing clipped, slow markers, a real displacement
    X11, U11 = mref.move(X0, c0, *mref.pose(m, 11))
    assert 5.9 < X11.min() and X11.max() < 18.2 and np.abs(U11).max() <= 0.071
    assert 0.7 < np.linalg.norm(X11.astype(np.float64) - X0, axis=1).max() < 0.8


def test_restated_loads():
    rng = np.random.default_rng(3)
    n = 700
    F = rng.normal(scale=1e-3, size=(n, 3)).astype(np.float32)
    A = rng.uniform(0.5, 1.5, n).astype(np.float32)
    X = rng.uniform(5, 19, (n, 3)).astype(np.float32)
    c = np.array([9.1, 10.2, 11.3])
    L = mref.loads(F, A, X, c)
    Fd, Ad, r = F.astype(np.float64), A.astype(np.float64), X.astype(np.float64) - c
    assert np.allclose(L[:3], -(Ad[:, None] * Fd).sum(axis=0), rtol=1e-12, atol=1e-15)
    assert np.allclose(L[3:], -(Ad[:, None] * np.cross(r, Fd)).sum(axis=0), rtol=1e-11, atol=1e-15)
    assert (np.abs(mref.loads_tree(F, A, X, c) - L) <= mref.loads_bound(F, A, X, c)).all()
