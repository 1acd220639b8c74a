"""Adjoint stepper: the discrete adjoint of the fused BGK step, for gradients of a loss through a run.

The reference differentiates its stepper through ``jax.grad`` and ships a Warp forward / backward stepper pair with checkpointing
(examples/out_of_core/autodiff_lbm.py).  This backend is ctypes plus hand-written HIP, so the backward pass is hand-written too
(csrc/adjoint_kernels.hpp, adjoint_step_kernel.hpp), pinned by the NumPy restatement tests/_adjoint_ref.py.

    forward = IncompressibleNavierStokesStepper(grid, boundary_conditions=[lid, walls])        # BGK, no force
    adjoint = AdjointStepper(forward)
    lam_out = adjoint.adjoint_step(f_n, lam_next, lam_out, bc_mask, missing_mask, omega)      # one step, cotangents in and out
    lam_0, other = adjoint.backward([f_0, .., f_{N-1}], lam_N, lam_other, bc_mask, missing_mask, omega)   # native sweep, no host wait
    lam_0, dL_domega = adjoint.gradient(f_init, bc_mask, missing_mask, omega, n_steps, cotangent, checkpoint_every=K)

One forward step is f_{n+1} = S(f_n; omega).  An adjoint step takes the forward state f_n and lam_{n+1} = dL/df_{n+1} and gives
lam_n = (dS/df_n)^T lam_{n+1}; its omega term sum_cells sum_l lam_l (feq_l - f*_l) is added on the device, in fp64 and a fixed order,
to a scalar that ``omega_gradient()`` reads and ``reset()`` clears.  The Jacobian is that of the exact-arithmetic map (casts count as
the identity).  Cotangent fields have the lattice's cardinality and the store dtype.  ``cotangent(f_final)`` returns lam_N as such a
field: ``MacroscopicAdjoint`` turns dL/drho and dL/du into it.

``gradient`` runs the forward pass with the forward stepper's native ``run``, keeps a checkpoint every ``checkpoint_every`` steps,
then walks the segments backwards: each is recomputed from its checkpoint into at most K - 1 scratch fields and swept by one native
``backward`` (``checkpoint_plan`` is the host logic).  Peak memory: ceil(N / K) + K population fields (f_init among them) and two
cotangent fields.

Scope: BGK; D2Q9, D3Q19, D3Q27; FP32FP32, FP64FP64, FP64FP32; periodic edges, EquilibriumBC, HalfwayBounceBackBC (a constant wall
velocity or none), FullwayBounceBackBC, DoNothingBC; single rank.  Limits (NotImplementedError at construction): KBC and
SmagorinskyLESBGK, a force vector, ZouHeBC / RegularizedBC / ExtrapolationOutflowBC, HybridBC, profile tables and time-dependent walls,
fp16 storage, slab-decomposed fields, IBMStepper and ScalarTransportStepper.  Not covered: gradients with respect to boundary values
or to geometry other than a PorousStepper's solidity (below), multi-rank sweeps, out-of-core checkpoints, an autograd wrapper (the DLPack
view of a field is enough to build one).

**Geometry.**  ``AdjointStepper(PorousStepper(...))`` is the adjoint of the porous step (porous_stepper.py) at the solidity field bound to
the forward stepper.  ``adjoint_step``, ``backward``, ``gradient`` and ``MacroscopicAdjoint`` work as above; every adjoint step also adds
each cell's term -omega sum_d B_d u_d to an fp64 field dL/dalpha on the device (the cell's own thread, in the order of the steps), which
``solidity_gradient()`` returns and ``reset()`` clears, and ``gradient`` returns three values: (lam_0, dL/domega, dL/dalpha)."""

from ... import _lib
from ..boundary_condition import DoNothingBC, EquilibriumBC, FullwayBounceBackBC, HalfwayBounceBackBC
from ...precision_policy import Precision
from .nse_stepper import IncompressibleNavierStokesStepper, refuse_unsupported
from .porous_stepper import PorousStepper


class AdjointStepper:
    def __init__(self, forward_stepper):
        fwd = forward_stepper
        if not isinstance(fwd, IncompressibleNavierStokesStepper):
            raise TypeError("AdjointStepper wraps an IncompressibleNavierStokesStepper")
        if type(fwd) not in (IncompressibleNavierStokesStepper, PorousStepper):
            raise NotImplementedError(f"AdjointStepper: the adjoint of {type(fwd).__name__} is not supported (the plain fluid stepper and "
                                      "PorousStepper only)")
        if fwd.collision_type != "BGK":
            raise NotImplementedError(f"AdjointStepper: collision_type {fwd.collision_type!r} is not supported; the adjoint is built for BGK")
        if fwd.force_vector is not None:
            raise NotImplementedError("AdjointStepper: a force vector is not supported")
        pp, grid = fwd.precision_policy, fwd.grid

        def known_kinds(bc):
            if type(bc) not in (EquilibriumBC, HalfwayBounceBackBC, FullwayBounceBackBC, DoNothingBC):
                raise NotImplementedError(f"AdjointStepper: {type(bc).__name__} is not supported (EquilibriumBC, HalfwayBounceBackBC, "
                                          "FullwayBounceBackBC and DoNothingBC only)")

        refuse_unsupported("AdjointStepper", pp, grid, fwd.boundary_conditions, also=known_kinds)
        self.forward = fwd
        self.grid = grid
        self.velocity_set = fwd.velocity_set
        self.precision_policy = pp
        self._ctx = fwd._ctx
        self.porous = type(fwd) is PorousStepper
        self._adjoint = None

    def _native(self):
        if self.porous:
            native = self.forward._bound()  # (refuses without a solidity field; the forward stepper's object: tables, alpha, gradients)
            if self._adjoint is None:
                self._adjoint = _PorousAdjoint(native)
            return self._adjoint
        if self._adjoint is None:
            fwd = self.forward
            descs = [bc._hip_descriptor() for bc in fwd.boundary_conditions]
            self._adjoint = _lib.Adjoint(self._ctx, self.velocity_set.hip_id, fwd._compute_code, fwd._store_code, descs)
        return self._adjoint

    def create_cotangent(self):
        """A zero cotangent field: the lattice's cardinality, the store dtype"""
        return self.grid.create_field(cardinality=self.velocity_set.q, dtype=self.precision_policy.store_precision, fill_value=0.0)

    def adjoint_step(self, f_n, lam_next, lam_out, bc_mask, missing_mask, omega):
        """lam_out = (dS/df_n)^T lam_next; adds the step's omega term to the device scalar"""
        self.forward.flush_deferred()
        self._native().step(f_n, lam_next, lam_out, bc_mask, missing_mask, omega)
        return lam_out

    def backward(self, states, lam_final, lam_other, bc_mask, missing_mask, omega):
        """The adjoint steps over ``states`` = [f_0 .. f_{N-1}], last first, in native code (one fused launch per step, nothing waits
        for the device); ``lam_final`` holds lam_N, both cotangent fields are overwritten.  Returns (lam_0, the other field)."""
        self.forward.flush_deferred()
        in_b = self._native().run(list(states), lam_final, lam_other, bc_mask, missing_mask, omega)
        return (lam_other, lam_final) if in_b else (lam_final, lam_other)

    def omega_gradient(self):
        """dL/domega of every adjoint step since the last reset (waits for the device)"""
        return self._native().omega_gradient()

    def solidity_gradient(self):
        """dL/dalpha of every adjoint step since the last reset, as a new fp64 field of one value per cell (a PorousStepper forward only;
        enqueued: reading the field waits for the device)"""
        if not self.porous:
            raise NotImplementedError("AdjointStepper.solidity_gradient: the forward stepper is not a PorousStepper")
        return self._native().solidity_gradient(self.grid.create_field(cardinality=1, dtype=Precision.FP64))

    def reset(self):
        """Clears dL/domega (and dL/dalpha of a porous forward stepper)"""
        self._native().reset()

    @staticmethod
    def checkpoint_plan(n_steps, checkpoint_every):
        """Host logic of ``gradient``: checkpoints at the steps 0, K, 2 K, .. < N; the segments [start, stop) in the order of the
        backward walk, each with the states it recomputes from its checkpoint (start + 1 .. stop - 1); the number of scratch fields;
        the peak number of live fields (checkpoints, f_init among them, + scratch + the two cotangent fields)."""
        n, k = int(n_steps), int(checkpoint_every)
        if n < 1 or k < 1:
            raise ValueError("n_steps and checkpoint_every must be at least 1")
        checkpoints = list(range(0, n, k))
        segments = [{"start": s, "stop": min(s + k, n), "recompute": list(range(s + 1, min(s + k, n)))} for s in reversed(checkpoints)]
        scratch = min(k, n)  # the forward pass' working pair and f_final, then the recomputed states of one segment (at most K - 1)
        return {"checkpoints": checkpoints, "segments": segments, "scratch_fields": scratch, "peak_fields": len(checkpoints) + scratch + 2,
                "forward_steps": n, "recomputed_steps": n - len(checkpoints)}

    def gradient(self, f_init, bc_mask, missing_mask, omega, n_steps, cotangent, checkpoint_every=8):
        """(lam_0 = dL/df_init, dL/domega[, dL/dalpha: a porous forward stepper]) of L(f_N), f_N = S^N(f_init; omega).
        ``cotangent(f_final)`` returns lam_N = dL/df_N as a field of the store dtype (it may read f_final, which is overwritten
        afterwards); the sweep takes that field over: lam_0 comes back in it or in a second one made here, and the other of the two is
        freed.  f_init is left as it is."""
        plan = self.checkpoint_plan(n_steps, checkpoint_every)
        fwd, store = self.forward, self.precision_policy.store_precision
        new = lambda: self.grid.create_field(cardinality=self.velocity_set.q, dtype=store)  # noqa: E731
        one_step = lambda src, dst, t: fwd.run(src, dst, bc_mask, missing_mask, omega, 1, first_timestep=t)  # noqa: E731  (src is kept)
        ckpt = {0: f_init}
        scratch = [new() for _ in range(plan["scratch_fields"])]
        lam_other = None
        try:
            # ---- forward: every segment from its checkpoint, the next checkpoint copied out of the working pair ----
            f_final = None
            for seg in reversed(plan["segments"]):
                start, stop = seg["start"], seg["stop"]
                last = stop == n_steps
                if stop - start == 1 and not last:
                    ckpt[stop] = new()
                    one_step(ckpt[start], ckpt[stop], start)
                    continue
                one_step(ckpt[start], scratch[0], start)
                cur = scratch[0]
                if stop - start > 1:
                    cur, _ = fwd.run(scratch[0], scratch[1], bc_mask, missing_mask, omega, stop - start - 1, first_timestep=start + 1)
                if last:
                    f_final = cur
                else:
                    ckpt[stop] = new()
                    ckpt[stop].copy_from(cur)
            lam = cotangent(f_final)
            lam_other = self.create_cotangent()
            self.reset()
            # ---- backward: recompute a segment's states from its checkpoint, sweep it ----
            for seg in plan["segments"]:
                states = [ckpt[seg["start"]]]
                for i, t in enumerate(seg["recompute"]):
                    one_step(states[-1], scratch[i], t - 1)
                    states.append(scratch[i])
                lam, lam_other = self.backward(states, lam, lam_other, bc_mask, missing_mask, omega)
                if seg["start"] != 0:
                    self._ctx.sync()  # (the sweep still reads the checkpoint)
                    ckpt.pop(seg["start"]).free()
            d_omega = self.omega_gradient()
            return (lam, d_omega, self.solidity_gradient()) if self.porous else (lam, d_omega)
        finally:
            self._ctx.sync()
            for f in scratch + [f for t, f in ckpt.items() if t != 0] + ([lam_other] if lam_other is not None else []):
                f.free()


class _PorousAdjoint:
    """The adjoint half of a native porous object (_lib.Porous) under the names of _lib.Adjoint"""

    def __init__(self, native):
        self.step, self.run = native.adjoint_step, native.adjoint_run
        self.omega_gradient, self.solidity_gradient, self.reset = native.omega_gradient, native.solidity_gradient, native.reset
