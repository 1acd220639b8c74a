"""NumPy restatement of k_ibm_move and of the per-body loads (xlb_amd/csrc/ibm_motion_kernels.hpp), test infrastructure only.

Elementwise operations only, in the kernels' stated order — no ``@``, no ``np.cross``, whose BLAS / fused paths might round
differently — so that ``move`` gives the kernel's bits.  ``loads`` adds the same fp64 terms in array order; the kernel adds them in
a tree, hence the bound ``loads_bound``: each of the two sums of n terms carries at most (n - 1) roundings of relative size 2^-53
applied to partial sums that never exceed sum |term|, so |kernel - restatement| <= 2 n 2^-53 sum |term| per component (the bound
tests/test_gpu_flow_statistics.py derives for its sums)."""

import numpy as np


def pose(motion, timestep):
    """(R (3, 3), c, w, v) float64 of a motion at a timestep."""
    R, c, w, v = motion.at(timestep)
    return tuple(np.asarray(a, dtype=np.float64) for a in (R, c, w, v))


def move(X0, centre0, R, c, w, v):
    """float32 reference positions (n, 3) -> (positions, velocities), both float32 (n, 3): X = c + R (X0 - c0) in fp64 as
    ((R_a0 d_0 + R_a1 d_1) + R_a2 d_2) + c_a, rounded to float32; U = v + w x (X_f32 - c), each cross-product component a b - c d."""
    X0 = np.asarray(X0, dtype=np.float32)
    d = [X0[:, a].astype(np.float64) - np.float64(centre0[a]) for a in range(3)]
    X = np.empty(X0.shape, np.float32)
    r = []
    for a in range(3):
        Xa = ((R[a, 0] * d[0] + R[a, 1] * d[1]) + R[a, 2] * d[2]) + c[a]
        X[:, a] = Xa.astype(np.float32)
        r.append(X[:, a].astype(np.float64) - c[a])
    U = np.empty(X0.shape, np.float32)
    U[:, 0] = (v[0] + (w[1] * r[2] - w[2] * r[1])).astype(np.float32)
    U[:, 1] = (v[1] + (w[2] * r[0] - w[0] * r[2])).astype(np.float32)
    U[:, 2] = (v[2] + (w[0] * r[1] - w[1] * r[0])).astype(np.float32)
    return X, U


def move_bodies(X0, U0, bodies, timestep):
    """``bodies``: list of (slice, motion or None, centre0).  Markers of moving bodies are placed, all others keep X0 / U0."""
    X, U = np.array(X0, dtype=np.float32), np.array(U0, dtype=np.float32)
    for sl, motion, centre0 in bodies:
        if motion is not None:
            X[sl], U[sl] = move(X0[sl], centre0, *pose(motion, timestep))
    return X, U


def load_terms(F, A, X, c):
    """(n, 6) float64: A F and A ((X - c) x F) per marker, every factor promoted to double before any product."""
    F, A, X = np.asarray(F).astype(np.float64), np.asarray(A).astype(np.float64), np.asarray(X).astype(np.float64)
    r = [X[:, a] - np.float64(c[a]) for a in range(3)]
    f = [F[:, a] for a in range(3)]
    return np.stack([A * f[0], A * f[1], A * f[2], A * (r[1] * f[2] - r[2] * f[1]), A * (r[2] * f[0] - r[0] * f[2]), A * (r[0] * f[1] - r[1] * f[0])],
                    axis=1)


def loads(F, A, X, c):
    """(6,) float64: the force -sum A F and the torque -sum A (X - c) x F on the body, the terms added in array order."""
    terms = load_terms(F, A, X, c)
    total = np.zeros(6)
    for row in terms:
        total = total + row
    return -total


def loads_bound(F, A, X, c):
    """(6,) the derived bound on |tree sum - sequential sum| per component: 2 n 2^-53 sum |term|."""
    terms = load_terms(F, A, X, c)
    return 2.0 * len(terms) * 2.0**-53 * np.abs(terms).sum(axis=0)


def loads_tree(F, A, X, c, chunk=256):
    """(6,) the bits k_ibm_loads / k_ibm_loads_combine produce for ONE body: chunks of 256 consecutive markers padded with zeros,
    inside a chunk neighbours added upwards level by level (all additions of a level at once, as the parallel kernel does them),
    then the chunks in index order."""
    terms = load_terms(F, A, X, c)
    total = np.zeros(6)
    for o in range(0, len(terms), chunk):
        part = np.zeros((chunk, 6))
        part[: len(terms[o : o + chunk])] = terms[o : o + chunk]
        s = 1
        while s < chunk:
            idx = np.arange(2 * s - 1, chunk, 2 * s)
            part[idx] = part[idx - s] + part[idx]
            s *= 2
        total = total + part[chunk - 1]
    return -total
