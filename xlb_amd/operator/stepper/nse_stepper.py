"""Incompressible Navier-Stokes stepper: one fused HIP kernel per time step.

Reference: xlb/operator/stepper/nse_stepper.py — constructor :65-97, ``prepare_fields``
:99-148, boundary processing :150-205, the step itself :237-282 (JAX order, the parity
target) / :427-476 (fused Warp kernel, the structural model).

    stepper = IncompressibleNavierStokesStepper(grid, boundary_conditions, collision_type="BGK")
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    for i in range(n):
        f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, omega, i)
        f_0, f_1 = f_1, f_0

``stepper.run(f_0, f_1, bc_mask, missing_mask, omega, n_steps)`` runs the same loop natively
(no per-step Python dispatch, which costs tens of microseconds per call in the reference's
``Operator.__call__``).

**Pairing of reference-style calls.**  The fast kernel advances TWO steps per pass (csrc/step2_kernel.hpp).  So that an
unmodified XLB driver — the loop above, every example of the reference (mlups_3d.py:237-238) — gets it too, a call on
fields the two-step kernel supports is DEFERRED: nothing is enqueued; when the next call arrives with the two
population fields swapped (same masks, same omega) both steps run as one fused pass, otherwise — any other use of either
field, ``ctx.sync()``, a different call — the deferred step runs first as a single step.  The results are bit-identical
to single steps.  After a fused pair the field that received step t+1 in the reference's protocol holds it only virtually
(the fused pass writes f(t+2) next to f(t), and the two field objects exchange their device buffers): if it is read
before the next call overwrites it, it is materialised through a temporary third field — also when one of the two masks is used
first (edited, read, freed): the step that is owed was issued with the masks as they were.  Fields exported through DLPack /
``__cuda_array_interface__`` are never deferred (their memory must stay put); ``backend_config={"lazy_pairs": False}``
switches the mechanism off.  call_pairing.py owns the protocol (``CallPairing``: ``call`` defers and fuses, ``flush_deferred`` runs
the deferred step alone, ``_Materialise`` hooks a virtual field) and steps through this stepper's ``_step`` / ``_step2``.

**Time-dependent walls.**  A HalfwayBounceBackBC / HybridBC with ``profile(cells, timestep)`` gets one profile table per timestep:
the host evaluates the profile and stages the values (``xlbhip_stepper_stage_bc_profiles``: a ring of device slots, asynchronous
copies on the compute stream) before the launch that reads them; the step from f(t) to f(t+1) uses ``profile(cells, t)``.  A
reference-style call stages its own timestep; a deferred call at t pairs only with a call at t + 1; ``run`` stages chunks of at most
half the ring and evaluates the next chunk while the device runs the current one."""

import time

import numpy as np

from ... import _lib
from ...compute_backend import ComputeBackend
from ...helper.check_boundary_overlaps import check_bc_overlaps
from ...helper.initializers import initialize_eq
from ...helper.nse_fields import create_nse_fields
from ...precision_policy import Precision
from ..boundary_condition import HybridBC, ImplementationStep
from ..boundary_masker import IndicesBoundaryMasker
from ..collision import BGK, KBC, RecursiveRegularizedBGK, RegularizedBGK, SmagorinskyLESBGK
from ..equilibrium import QuadraticEquilibrium
from ..macroscopic import Macroscopic
from ..operator import Operator
from ..stream import Stream
from .call_pairing import CallPairing, drop_virtual_destination, pairs_in_time  # noqa: F401 (pairs_in_time: imported from here too)
from .stepper import Stepper


def refuse_unsupported(name, precision_policy, grid, boundary_conditions=(), hybrid="HybridBC is not supported", also=None):
    """What the steppers beside the plain fluid step refuse at construction, worded alike: fp16 storage, slab-decomposed fields; then
    per boundary condition HybridBC, a profile and what the caller checks `also` (one BC at a time: the refusals keep the list's order)."""
    if precision_policy.store_precision is Precision.FP16:
        raise NotImplementedError(f"{name}: fp16 storage ({precision_policy.name}) is not supported; use FP32FP32, FP64FP64 or FP64FP32")
    if getattr(grid, "halo", 0) != 0 or getattr(grid, "n_ranks", 1) != 1:
        raise NotImplementedError(f"{name}: slab-decomposed fields (ghost planes, several ranks) are not supported")
    for bc in boundary_conditions:
        if isinstance(bc, HybridBC):
            raise NotImplementedError(f"{name}: {hybrid}")
        if getattr(bc, "profile", None) is not None or getattr(bc, "is_time_dependent", False):
            raise NotImplementedError(f"{name}: {type(bc).__name__} with a profile (per-cell or time-dependent values) is not supported")
        if also is not None:
            also(bc)


REGULARIZED_COLLISIONS = ("RegularizedBGK", "RecursiveRegularizedBGK")


def refuse_regularized(name, collision_type):
    """The steppers with a coupled kernel of their own have no regularised form of it."""
    if collision_type in REGULARIZED_COLLISIONS:
        raise NotImplementedError(f"{name}: collision_type {collision_type!r} is not supported; the coupled step is built for BGK, KBC and "
                                  "SmagorinskyLESBGK")


def chunk_plan(n_steps, ring_slots):
    """Chunk sizes of a run with time-dependent walls: at most half the ring (the next chunk is staged while the device still reads
    this one's tables) and even, so that pairs of steps stay pairs; only the last chunk may be odd.  (Chunks that start at 2 and
    double measured slower at 512^3 — the device idles at every doubling: profiles/time_dependent_walls.md.)"""
    size = max(2, (int(ring_slots) // 2) & ~1)
    n = int(n_steps)
    return [min(size, n - i) for i in range(0, n, size)]


class IncompressibleNavierStokesStepper(Stepper):
    def __init__(self, grid, boundary_conditions=[], collision_type="BGK", streaming_scheme="pull",
                 forcing_scheme="exact_difference", force_vector=None, backend_config={}):
        self.backend_config = dict(backend_config or {})
        self.collision_type = collision_type
        self.streaming_scheme = streaming_scheme
        if streaming_scheme != "pull":
            raise AssertionError(f"Unknown or unimplemented streaming scheme for backend: {ComputeBackend.HIP}")
        if force_vector is not None:
            if forcing_scheme != "exact_difference":
                raise NotImplementedError(f"Force model {forcing_scheme} not implemented!")  # forced_collision.py:40
            force_vector = np.asarray(force_vector, dtype=np.float64)
        self.forcing_scheme = forcing_scheme
        self.force_vector = force_vector
        self._native = None
        self._td_bcs, self._td_slots = [], 0  # BCs with time-dependent wall velocities (declaration order) and the ring's slot count
        self._pairing = CallPairing(self) if self.backend_config.get("lazy_pairs", True) else None
        super().__init__(grid, boundary_conditions)
        vs, pp, be = self.velocity_set, self.precision_policy, self.compute_backend
        if collision_type == "BGK":
            self.collision = BGK(vs, pp, be)
        elif collision_type == "KBC":
            self.collision = KBC(vs, pp, be)
        elif collision_type == "SmagorinskyLESBGK":
            self.collision = SmagorinskyLESBGK(vs, pp, be)
        elif collision_type in REGULARIZED_COLLISIONS:
            # single-step kernel, three precision policies, one rank (slab grids are untested with it: refused)
            refuse_unsupported(f"collision_type {collision_type!r}", pp, grid)
            self.collision = (RegularizedBGK if collision_type == "RegularizedBGK" else RecursiveRegularizedBGK)(vs, pp, be)
        else:
            raise NotImplementedError(f"collision_type {collision_type!r} is not available on the HIP backend "
                                      "(BGK, KBC, SmagorinskyLESBGK, RegularizedBGK, RecursiveRegularizedBGK)")
        if force_vector is not None and force_vector.shape != (vs.d,):
            raise AssertionError("Check the dimensions of the input force!")  # forced_collision.py:41
        self.stream = Stream(vs, pp, be)
        self.equilibrium = QuadraticEquilibrium(vs, pp, be)
        self.macroscopic = Macroscopic(vs, pp, be)

    # -- native stepper object, created lazily (BC ids and constants are final by then)
    def _native_stepper(self):
        if self._native is None:
            descs = [bc._hip_descriptor() for bc in self.boundary_conditions]
            self._native = _lib.Stepper(self._ctx, self.velocity_set.hip_id, self.collision.hip_collision_id, self._compute_code,
                                        self._store_code, descs)
            if isinstance(self.collision, SmagorinskyLESBGK):
                self._native.set_smagorinsky(self.collision.smagorinsky_coef)
            for bc in self.boundary_conditions:
                table = bc._profile_table(self.grid) if hasattr(bc, "_profile_table") else None
                if table is not None:
                    self._native.set_bc_profile(bc.id, *table)
            for bc in self.boundary_conditions:
                keys = getattr(bc, "_td_keys", None) if getattr(bc, "is_time_dependent", False) else None
                if keys is not None and keys.size > 0:
                    self._native.set_bc_profile_cells(bc.id, keys)
                    self._td_bcs.append(bc)
            if self._td_bcs:
                self._td_slots = self._native.profile_slots()
            for bc in self.boundary_conditions:
                table = getattr(bc, "_distance_table", None)
                if table is not None:
                    # wall-distance weights the mesh masker gathered (HybridBC with use_mesh_distance); interior linear
                    # cell index == storage cell index on the single-rank fields mesh BCs live on
                    self._native.set_bc_distances(*table)
            if self.force_vector is not None:
                self._native.set_force(self._internal3(self.force_vector))
        return self._native

    def _internal3(self, v):
        """A d-component vector (or None) in the internal 3-component form."""
        return None if v is None else np.concatenate([np.zeros(3 - self.velocity_set.d), np.asarray(v, dtype=np.float64)])

    def prepare_fields(self, initializer=None):
        _, f_0, f_1, missing_mask, bc_mask = create_nse_fields(
            grid=self.grid, velocity_set=self.velocity_set, compute_backend=self.compute_backend, precision_policy=self.precision_policy
        )
        f_1, bc_mask, missing_mask = self._process_boundary_conditions(self.boundary_conditions, f_1, bc_mask, missing_mask)
        if initializer is not None:
            f_0 = initializer(bc_mask, f_0)
        else:
            f_0 = initialize_eq(f_0, self.grid, self.velocity_set, self.precision_policy, self.compute_backend)
        return f_0, f_1, bc_mask, missing_mask

    def _process_boundary_conditions(self, boundary_conditions, f_1, bc_mask, missing_mask):
        import weakref

        for bc in boundary_conditions:
            bc._stepper_ref = weakref.ref(self)  # (MomentumTransfer of a HybridBC / profile wall reads this stepper's tables)
        check_bc_overlaps(boundary_conditions, self.velocity_set.d, self.compute_backend)
        masker = IndicesBoundaryMasker(self.velocity_set, self.precision_policy, self.compute_backend, grid=self.grid)
        with_indices = [bc for bc in boundary_conditions if getattr(bc, "indices", None) is not None]
        if with_indices:
            bc_mask, missing_mask = masker(with_indices, bc_mask, missing_mask)
        # mesh-based BCs (nse_stepper.py:165-203 in the reference): one masker per voxelisation method
        for bc in boundary_conditions:
            if getattr(bc, "mesh_vertices", None) is None:
                continue
            from ..boundary_masker import mesh_masker_for

            mesh_masker = mesh_masker_for(getattr(bc, "voxelization_method", None), self.velocity_set, self.precision_policy, self.compute_backend)
            f_1, bc_mask, missing_mask = mesh_masker(bc, f_1, bc_mask, missing_mask)
        # wall-velocity profiles (HybridBC(profile=...), bc_hybrid.py:163-172): evaluated at the BC's cells, known only now
        with_profile = [bc for bc in boundary_conditions if callable(getattr(bc, "_evaluate_profile", None)) and getattr(bc, "profile", None)]
        if with_profile:
            if bc_mask.halo != 0:
                raise NotImplementedError("wall-velocity profiles need fields without ghost planes (single rank)")
            ids = bc_mask.numpy()[0]
            if ids.ndim == 2:
                ids = ids[None]
            for bc in with_profile:
                cells = np.argwhere(ids == bc.id).T  # (3, n), ascending storage order
                keys = (cells[0] * ids.shape[1] + cells[1]) * ids.shape[2] + cells[2]
                bc._evaluate_profile(cells, keys)
        return f_1, bc_mask, missing_mask

    @Operator.register_backend(ComputeBackend.HIP)
    def hip_implementation(self, f_0, f_1, bc_mask, missing_mask, omega, timestep):
        if self._pairing is None:
            drop_virtual_destination(f_1)  # (another stepper's pair may have left it virtual; this step overwrites it)
        if self._pairing is None or not self._pairing.call(f_0, f_1, bc_mask, missing_mask, omega, timestep):
            self._step(f_0, f_1, bc_mask, missing_mask, omega, timestep)
        return f_0, f_1

    # -- time-dependent wall velocities (module docstring) ---------------------------------------------------------
    def _time_dependent_bcs(self):
        self._native_stepper()
        return self._td_bcs

    def _td_rows(self, t_first, n):
        """(n, cells, 3) wall velocities of the time-dependent BCs' cells (declaration order) at t_first .. t_first + n - 1, written in
        place into ONE staging buffer that every call reuses (stage_bc_profiles has copied the previous rows when it returned)."""
        sizes = [bc._td_keys.size for bc in self._td_bcs]
        buf = getattr(self, "_td_buf", None)
        if buf is None or buf.shape[0] < n:
            buf = self._td_buf = np.empty((max(n, self._td_slots // 2), sum(sizes), 3))
        rows = buf[:n]
        for k in range(n):
            o = 0
            for bc, m in zip(self._td_bcs, sizes):
                bc.profile_at(int(t_first) + k, out=rows[k, o : o + m])
                o += m
        return rows

    def _stage(self, t_first, n):
        """Evaluate and stage the tables of timesteps t_first .. t_first + n - 1 (nothing without time-dependent walls)."""
        if self._time_dependent_bcs():
            self._native.stage_bc_profiles(int(t_first), self._td_rows(t_first, n))

    # -- pairing of reference-style calls (module docstring): call_pairing.py owns it and steps through these --------
    def _step(self, f_src, f_dst, bc_mask, missing_mask, omega, t):
        """Stage timestep t's tables, then one native step."""
        self._stage(t, 1)
        self._native_stepper().step(f_src, f_dst, bc_mask, missing_mask, omega, t)

    def _step2(self, f_src, f_dst, bc_mask, missing_mask, omega, t):
        """Stage the tables of t and t + 1, then one fused pass: f(t) in f_src -> f(t+2) in f_dst."""
        self._stage(t, 2)
        self._native_stepper().step2(f_src, f_dst, bc_mask, missing_mask, omega, t)

    def _step2_eligible(self, f_src, f_dst, bc_mask, missing_mask):
        return self._native_stepper().step2_eligible(f_src, f_dst, bc_mask, missing_mask)

    def _temporary_field(self):
        return self.grid.create_field(cardinality=self.velocity_set.q, dtype=self.precision_policy.store_precision)

    _deferred = property(lambda self: self._pairing.deferred if self._pairing else None)  # (read-only views: tests, diagnostics)
    _n_fused_pairs = property(lambda self: self._pairing.n_fused_pairs if self._pairing else 0)
    _n_materialised = property(lambda self: self._pairing.n_materialised if self._pairing else 0)

    def flush_deferred(self):
        """Enqueue a deferred reference-style call as a single step (its fields are about to be used another way)."""
        if self._pairing is not None:
            self._pairing.flush_deferred()

    def abandon_deferred(self):
        """Forget a deferred reference-style call and unhook its fields: its step will never run."""
        if self._pairing is not None:
            self._pairing.abandon_deferred()

    def _run_loop(self, f_0, f_1, n_steps):
        """What run and run_timed begin with: the deferred call runs first, a virtual destination is dropped; then the loop that
        interleaves host work with the device's — host-staged ghost planes, chunks of time-dependent tables — or None: the native loop."""
        self.flush_deferred()
        drop_virtual_destination(f_1, n_steps)
        if f_0.halo > 0 and self._ctx.get_option("external_halo"):
            return self._run_host_staged
        return self._run_chunked if self._time_dependent_bcs() else None

    def run(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """``n_steps`` x (step, swap) in native code; returns (f_current, f_other)."""
        loop = self._run_loop(f_0, f_1, n_steps)
        if loop is not None:
            return loop(f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep)
        in_b = self._native_stepper().run(f_0, f_1, bc_mask, missing_mask, omega, first_timestep, n_steps)
        return (f_1, f_0) if in_b else (f_0, f_1)

    def run_timed(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep=0):
        """As :meth:`run`; also returns the device time in ms measured with HIP events.  (Host-staged transports and time-dependent
        walls: the wall clock between two synchronisations — those loops interleave host work with the device's.)"""
        loop = self._run_loop(f_0, f_1, n_steps)
        if loop is not None:
            self._ctx.sync()  # no single native loop to bracket with events; wall clock instead
            t0 = time.perf_counter()
            out = loop(f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep)
            self._ctx.sync()
            return out, (time.perf_counter() - t0) * 1e3
        in_b, ms = self._native_stepper().run_timed(f_0, f_1, bc_mask, missing_mask, omega, first_timestep, n_steps)
        return ((f_1, f_0) if in_b else (f_0, f_1)), ms

    def _run_chunked(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep):
        """The native run loop in chunks (chunk_plan) for a stepper with time-dependent walls: every chunk's tables are staged before
        its xlbhip_run_any, and the next chunk's profiles are evaluated while the device runs this one (nothing here waits for it).

        A profile that raises in the first chunk stops the run before anything is enqueued.  One that raises later leaves the chunks
        before it enqueued: the exception then carries ``timestep_reached`` (the run holds f(t) for that t) and ``fields`` = (the field
        holding it, the other one), and its message says so."""
        native = self._native
        cur, oth, t = f_0, f_1, int(first_timestep)
        plan = chunk_plan(n_steps, self._td_slots)
        rows = self._td_rows(t, plan[0]) if plan else None
        for i, k in enumerate(plan):
            native.stage_bc_profiles(t, rows)
            if native.run(cur, oth, bc_mask, missing_mask, omega, t, k):
                cur, oth = oth, cur
            t += k
            if i + 1 < len(plan):
                try:
                    rows = self._td_rows(t, plan[i + 1])
                except Exception as e:
                    where = "f_0" if cur is f_0 else "f_1"
                    e.timestep_reached, e.fields = t, (cur, oth)
                    e.args = (f"{e.args[0] if e.args else e} (the run stopped at timestep {t}: f({t}) is in the field passed as {where})",) + e.args[1:]
                    raise
        return cur, oth

    def _momentum_transfer(self, bc, f_0, bc_mask, missing_mask, timestep=0):
        """MomentumTransfer of a HybridBC / profile wall of this stepper; a time-dependent wall with its velocities at `timestep`."""
        native = self._native_stepper()
        if bc not in self._td_bcs:
            return native.momentum_transfer(bc.id, f_0, bc_mask, missing_mask)
        for fld in (f_0, bc_mask, missing_mask):
            fld.handle  # (deferred work on these fields runs first: it stages its own tables)
        self._stage(timestep, 1)
        return native.momentum_transfer_at(bc.id, timestep, f_0, bc_mask, missing_mask)

    def _run_host_staged(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep):
        """The native run loop with the ghost planes moved by the host (``init_process_group(transport="host")``):
        same kernels and the same pairing of steps as ``xlbhip_run``, the debugging transport in between."""
        from ...distribute import HostStagedHalo, all_reduce_min

        if self._time_dependent_bcs():
            raise NotImplementedError("time-dependent wall-velocity profiles run on a single rank (fields without ghost planes)")
        native = self._native_stepper()
        halo = HostStagedHalo(self.grid, self.velocity_set)
        cur, oth, i = f_0, f_1, 0
        fuse = f_0.halo >= 2 and n_steps >= 2 and native.step2_eligible(cur, oth, bc_mask, missing_mask)
        # the message plan differs between pairs and single steps: the decision must be the same on every rank
        # (uneven slabs may sit on either side of the two-step kernel's chip-filling rule)
        fuse = bool(all_reduce_min(1.0 if fuse else 0.0))
        if fuse and bc_mask is not None and self.boundary_conditions:
            halo.exchange_masks(bc_mask, missing_mask)
        while i < n_steps:
            if fuse and n_steps - i >= 2:
                halo.exchange(cur, depth=2)
                native.step2(cur, oth, bc_mask, missing_mask, omega, first_timestep + i)
                i += 2
            else:
                halo.exchange(cur, depth=1)
                native.step(cur, oth, bc_mask, missing_mask, omega, first_timestep + i)
                i += 1
            cur, oth = oth, cur
        return cur, oth

    @property
    def has_post_streaming_bc(self):
        return any(bc.implementation_step == ImplementationStep.STREAMING for bc in self.boundary_conditions)
