"""FlowStatistics: running means, profiles and a blow-up watchdog, accumulated on the device.

The reference has no such operator; its drivers download whole fields and reduce them in NumPy.  Here a sample is one pass over
the populations that is enqueued like a step, so it can follow ``stepper.run`` without a host synchronisation:

    stats = FlowStatistics(grid, keep_axes=(2,), exclude_ids=(255,), order=2)
    for _ in range(n):
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, k)
        stats.sample(f_0, bc_mask)      # enqueued on the compute stream; nothing is read back
    r = stats.result()                  # synchronises: dict of float64 NumPy arrays shaped like the kept axes
    stats.reset()

Per sampled cell rho and u are what ``Macroscopic`` writes (compute dtype); they are promoted to double and every product and sum
is taken in double.  Channels with ``order=2``: count, rho, rho^2, u_a, u_a u_b in the order of ``SecondMoment`` (xx, xy, xz, yy, yz,
zz; three in 2-D) — 12 in 3-D, 8 in 2-D; ``order=1`` keeps count, rho and u_a.

``keep_axes``: the grid axes that are kept, all others are summed over: ``()`` global scalars, ``(2,)`` the wall-normal profile of a
channel, ``(0,)`` streamwise development, ``(0, 1, 2)`` a running mean of the full field.  The running sums take channels x 8 bytes
per BIN of device memory — with ``(0, 1, 2)`` that is 96 bytes per cell (12.9 GB at 512^3), more than the populations themselves.
Results are shaped like the kept axes in ascending order.

``exclude_ids``: ``bc_mask`` values whose cells are not sampled (default: 255, solid).  ``sample(f, None)`` samples every cell.  The
count channel says how many cells a bin holds, so a mean is sum / count.

Watchdog (``result()["max_u2"]``, ``["nonfinite_last"]``, ``["nonfinite_total"]``): the largest u.u of the sampled cells of the last
sample, and the number of sampled cells whose rho or u is not finite.  Such a cell adds to that number and to nothing else, so one
bad cell does not turn every sum into NaN.

The sums are bit-identical from run to run, object to object and device to device: no floating-point atomics; which cells meet in
which partial sum and the order the partial sums are added in depend on the local shape, ``keep_axes`` and ``order`` only
(csrc/stats_kernels.hpp).  Fields with ghost planes are accepted and ghost planes are never sampled.  With several ranks
``result()`` adds the ranks' sums (in rank order, through the host collective of ``xlb_amd.distribute``) when x is summed over; when
x is kept it returns this rank's rows, which start at ``grid.x_offset``.  The watchdog's numbers cover all ranks either way."""

import numpy as np

from ... import _lib
from ...compute_backend import ComputeBackend
from ..operator import Operator


def channel_names(d, order):
    """Names of the channels of the raw sums, in storage order."""
    comps = "xyz"[:d]
    names = ["count", "rho"] + (["rho2"] if order == 2 else []) + ["u" + a for a in comps]
    if order == 2:
        names += ["u" + comps[a] + "u" + comps[b] for a in range(d) for b in range(a, d)]
    return names


def means_from_sums(sums, samples, d, order):
    """The means ``result()`` returns, from raw sums shaped (channels, *bins).  Bins without cells give NaN."""
    sums = np.asarray(sums, np.float64)
    if sums.shape[0] != len(channel_names(d, order)):
        raise ValueError(f"{sums.shape[0]} channels given, order {order} in {d}-D has {len(channel_names(d, order))}")
    n = sums[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"count": n / samples if samples else np.zeros_like(n), "rho": sums[1] / n}
        if order == 2:
            out["rho2"] = sums[2] / n
            out["u"] = sums[3 : 3 + d] / n
            out["uu"] = sums[3 + d :] / n
        else:
            out["u"] = sums[2 : 2 + d] / n
    out["sums"] = sums
    return out


def reynolds_stress_from_means(u, uu):
    """<u_a u_b> - <u_a><u_b> in the component order of ``uu``."""
    d = u.shape[0]
    pairs = [(a, b) for a in range(d) for b in range(a, d)]
    return np.stack([uu[k] - u[a] * u[b] for k, (a, b) in enumerate(pairs)])


class FlowStatistics(Operator):
    def __init__(self, grid, keep_axes=(), exclude_ids=(255,), order=2, velocity_set=None, precision_policy=None, compute_backend=None):
        super().__init__(velocity_set, precision_policy, compute_backend)
        self.grid = grid
        dim = len(grid.shape)
        if dim != self.velocity_set.d:
            raise ValueError(f"FlowStatistics: a {dim}-D grid with the {self.velocity_set.d}-D lattice {type(self.velocity_set).__name__}")
        axes = tuple(int(a) for a in keep_axes)
        if any(a < 0 or a >= dim for a in axes):
            raise ValueError(f"FlowStatistics: keep_axes {tuple(keep_axes)} out of range for a {dim}-D grid (axes 0 .. {dim - 1})")
        if len(set(axes)) != len(axes):
            raise ValueError(f"FlowStatistics: keep_axes {tuple(keep_axes)} names an axis twice")
        if order not in (1, 2):
            raise ValueError(f"FlowStatistics: order must be 1 or 2, not {order!r}")
        ids = tuple(int(v) for v in exclude_ids)
        if any(v < 0 or v > 255 for v in ids):
            raise ValueError(f"FlowStatistics: exclude_ids {ids} are not bc_mask values (0 .. 255)")
        self.keep_axes = tuple(sorted(axes))
        self.exclude_ids = tuple(sorted(set(ids)))
        self.order = int(order)
        self.local_shape = tuple(getattr(grid, "local_shape", grid.shape))
        self.n_ranks = int(getattr(grid, "n_ranks", 1))
        # 2-D grids are stored as one x plane: grid axes 0, 1 are storage y, z
        self._shape3 = ((1,) + self.local_shape) if dim == 2 else self.local_shape
        self._keep_mask = sum(1 << (a + 3 - dim) for a in self.keep_axes)
        self.bins_shape = tuple(self.local_shape[a] for a in self.keep_axes)
        self.channels = channel_names(dim, self.order)
        self._native = None

    # -- the native object is made with the first sample: constructing the operator needs no device
    def _stats(self):
        if self._native is None:
            self._native = _lib.Stats(self._ctx, self.velocity_set.hip_id, self._compute_code, self._shape3, self._keep_mask, self.order, self.exclude_ids)
        return self._native

    def _check_fields(self, f, bc_mask):
        q = self.velocity_set.q
        if not isinstance(f, _lib.Field) or f.dtype_code not in (_lib.F64, _lib.F32, _lib.F16):
            raise ValueError(f"FlowStatistics.sample: f must be a population field (float, {q} components), got {f!r}")
        if f.cardinality != q:
            raise ValueError(f"FlowStatistics.sample: a field of {f.cardinality} components is not a {type(self.velocity_set).__name__} population field ({q})")
        if f.grid_shape != self.local_shape:
            raise ValueError(f"FlowStatistics.sample: field of shape {f.grid_shape}, the statistics were made for {self.local_shape}")
        if bc_mask is not None:
            if not isinstance(bc_mask, _lib.Field) or bc_mask.dtype_code != _lib.U8 or bc_mask.cardinality != 1:
                raise ValueError(f"FlowStatistics.sample: bc_mask must be a one-component uint8 field, got {bc_mask!r}")
            if bc_mask.grid_shape != f.grid_shape:
                raise ValueError(f"FlowStatistics.sample: bc_mask of shape {bc_mask.grid_shape} lives on another grid than f {f.grid_shape}")

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f, bc_mask=None):
        self._check_fields(f, bc_mask)
        self._stats().sample(f, bc_mask)
        return self

    def sample(self, f, bc_mask=None):
        """Add one sample of ``f`` to the running sums.  Enqueued on the compute stream: no host synchronisation, no host read."""
        return self.hip_implementation(f, bc_mask)

    @property
    def samples(self):
        """Samples since the last reset (a host counter)."""
        return 0 if self._native is None else self._native.samples

    def reset(self):
        if self._native is not None:
            self._native.reset()

    def _reduce_ranks(self, sums, umax, bad_last, bad_total):
        if self.n_ranks <= 1:
            return sums, umax, bad_last, bad_total
        from ... import distribute

        if not self._keep_mask & 1:
            total = np.zeros_like(sums)
            for part in distribute.all_gather(sums):  # rank order: the same bits on every rank
                total = total + np.asarray(part, np.float64).reshape(sums.shape)
            sums = total
        w = distribute.all_gather([float(umax), int(bad_last), int(bad_total)])
        return sums, max(x[0] for x in w), sum(x[1] for x in w), sum(x[2] for x in w)

    def result(self):
        """Synchronises and returns the means over cells and samples: "count" (cells per bin and sample), "rho", "rho2", "u" (d, ...),
        "uu" (n_pi, ...), the raw "sums" (channels, ...) and "samples", "max_u2", "nonfinite_last", "nonfinite_total"."""
        nc = len(self.channels)
        n_bins = int(np.prod(self.bins_shape, dtype=np.int64)) if self.bins_shape else 1
        if self._native is None:
            sums, samples, umax, bad_last, bad_total = np.zeros(nc * n_bins), 0, 0.0, 0, 0
        else:
            sums, samples, umax, bad_last, bad_total = self._native.read(nc * n_bins)
        sums = sums.reshape((nc,) + self.bins_shape)
        sums, umax, bad_last, bad_total = self._reduce_ranks(sums, umax, bad_last, bad_total)
        out = means_from_sums(sums, samples, len(self.grid.shape), self.order)
        out.update(samples=samples, max_u2=umax, nonfinite_last=bad_last, nonfinite_total=bad_total)
        return out

    def reynolds_stress(self, result=None):
        """<u_a u_b> - <u_a><u_b>, shaped (n_pi, ...) in the order of "uu" (``order=2`` only).  ``result``: a dict from :meth:`result`
        to work from instead of reading the device again."""
        if self.order != 2:
            raise ValueError("FlowStatistics.reynolds_stress needs order=2 (the second moments are not accumulated with order=1)")
        r = self.result() if result is None else result
        return reynolds_stress_from_means(r["u"], r["uu"])
