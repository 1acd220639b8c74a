"""Pairing of reference-style calls: the one owner of the protocol that nse_stepper.py's docstring and DESIGN.md §3 "Pairing" describe.

No library here: fields are used through ``_lib.HookedBuffer`` plus ``halo``, ``info()`` and ``dtype``, the rest through the object handed to
``CallPairing`` (the stepper, or the recording stand-in of tests/test_call_pairing_host.py): ``_step(f_src, f_dst, bc_mask, missing_mask, omega, t)``
stages t's tables and runs one native step, ``_step2(...)`` stages t and t + 1 and runs one fused pass, ``_step2_eligible(f_src, f_dst, bc_mask,
missing_mask)``, ``_time_dependent_bcs()``, ``_temporary_field()`` (a new population field), ``_ctx.mem_info()`` and ``_ctx.defers_work(obj)``."""

import weakref


def pairs_in_time(t_deferred, timestep, time_dependent):
    """May a deferred call at t_deferred be fused with a call at `timestep`?  Always without time-dependent walls (the timestep does not
    enter the step); with them only when the call is the next timestep — the fused pair runs steps t and t + 1."""
    return not time_dependent or int(timestep) == int(t_deferred) + 1


class _Materialise:
    """Hook of a field that holds f(t+1) only virtually after a fused pair (its buffer holds f(t)): see CallPairing.call.  The step that is
    owed was issued with the masks as they were, so the two masks carry a hook of their own (_MasksOfVirtual) that leads here: whoever
    uses a mask first — to edit it, to free it, to read it — makes the step run first.  References go one way only, field -> this hook
    -> masks -> (weakly) field: a field abandoned while virtual is released at once, with its device memory, not by the cycle collector."""

    def __init__(self, pairing, stepper, field, bcm, miss, omega, t):
        self.args = (pairing, stepper, bcm, miss, omega, t)
        self.of_masks = _MasksOfVirtual(field)
        for fld in (field, bcm, miss):
            if fld is not None and fld.hook is not None:
                fld.handle  # (whatever else is owed on it runs first; a pair has just used all three, so normally nothing is)
        field.hook_with(self)
        self._hook_masks()

    def _hook_masks(self):
        for mask in self.args[2:4]:
            if mask is not None and mask.hook is None:
                mask.hook_with(self.of_masks)

    def drop(self, field):
        """Nothing is owed any more (the step ran, or the field is about to be overwritten)."""
        field.unhook(self)
        for mask in self.args[2:4]:
            if mask is not None:
                mask.unhook(self.of_masks)

    def __call__(self, field):
        pairing, stepper, bcm, miss, omega, t = self.args
        self.drop(field)
        try:
            pairing._materialise(stepper, field, bcm, miss, omega, t)
        except BaseException:
            self._hook_masks()  # still owed, whichever of the three is used next (HookedBuffer.handle puts the field's hook back)
            raise


class _MasksOfVirtual:
    """Hook of the two masks while a field is virtual (_Materialise): using a mask uses that field first."""

    def __init__(self, field):
        self.field = weakref.ref(field)

    def __call__(self, _mask):
        field = self.field()
        if field is not None and is_virtual(field) and field.hook.of_masks is self:
            field.handle


def is_virtual(field):
    """Does the field hold its f(t+1) only virtually (a fused pair passed it by and nobody has looked since)?"""
    return isinstance(field.hook, _Materialise)


def drop_virtual_destination(f_1, n_steps=1):
    """The first of n >= 1 steps overwrites f_1 entirely: a virtual f(t+1) in it (left by a fused pair of reference-style
    calls) needs no materialisation — which would allocate a third field and run an extra step for nothing."""
    if n_steps >= 1 and is_virtual(f_1):
        f_1.hook.drop(f_1)


class CallPairing:
    def __init__(self, stepper):
        # weakly: the stepper owns this object, and a cycle would leave the native stepper's device memory to the cycle collector.
        # What is owed keeps the stepper alive, as it always did: the deferred record (_owed_by) and a virtual field's hook hold it.
        self._stepper = weakref.ref(stepper)
        self.deferred = self._owed_by = None  # (f_src, f_dst, bc_mask, missing_mask, omega, timestep): a step not enqueued yet
        self.n_fused_pairs = self.n_materialised = 0  # statistics of the pairing (tests, diagnostics)
        self._room_calls, self._room_ok = 0, None

    def call(self, f_0, f_1, bc_mask, missing_mask, omega, timestep):
        """True when this call was absorbed (deferred, or executed as the second half of a fused pair)."""
        stepper = self._stepper()
        drop_virtual_destination(f_1)  # about to be overwritten: nothing to materialise
        d = self.deferred
        if d is not None:
            f_src, f_dst, bcm, miss, om, t = d
            if (f_0 is f_dst and f_1 is f_src and bc_mask is bcm and missing_mask is miss and float(omega) == om and not (f_0._pinned or f_1._pinned)
                    and pairs_in_time(t, timestep, bool(stepper._time_dependent_bcs()))):
                # the caller swapped the fields: steps t and t + 1 in one pass, f(t) in f_src's buffer -> f(t+2) in f_dst's
                self.abandon_deferred()
                if not stepper._step2_eligible(f_src, f_dst, bcm, miss):  # (an option changed in between)
                    stepper._step(f_src, f_dst, bcm, miss, om, t)
                    return False
                stepper._step2(f_src, f_dst, bcm, miss, om, t)
                self.n_fused_pairs += 1
                # the reference's protocol leaves f(t+2) in THIS call's f_1 (= f_src) and f(t+1) in its f_0 (= f_dst):
                # exchange the buffers; f_dst now holds f(t) instead of f(t+1) until someone looks
                f_src.exchange_buffers(f_dst)
                _Materialise(self, stepper, f_dst, bcm, miss, om, t)  # (hooks f_dst and both masks: an edited mask must not reach that step)
                return True
            self.flush_deferred()
        # (step2_eligible is asked every time: the answer follows the backend options — fuse2, ... — and the masks' contents; host logic only)
        if (f_0.halo != 0 or f_0._pinned or f_1._pinned or not stepper._step2_eligible(f_0, f_1, bc_mask, missing_mask)
                or not self._room_for_a_third_field(stepper, f_0)):
            return False
        # defer: whoever touches either field first (or ctx.sync()) makes it run
        if f_0.hook is not None:  # the source itself is virtual (read it properly first)
            f_0.handle
        self._owe(stepper, (f_0, f_1, bc_mask, missing_mask, float(omega), timestep))
        stepper._ctx.defers_work(self)
        return True

    def _owe(self, stepper, d):
        self.deferred, self._owed_by = d, stepper
        for fld in d[:4]:  # the masks too: editing them must not overtake the deferred step
            if fld is not None:
                fld.hook_with(self.flush_deferred)

    def abandon_deferred(self):
        """Forget the deferred step and unhook its fields (it is about to run another way, or its caller gave up)."""
        d, self.deferred, self._owed_by = self.deferred, None, None
        for fld in (d or ())[:4]:
            if fld is not None:
                fld.unhook()

    def flush_deferred(self, *_):
        """Enqueue the deferred step as a single step (some other use of its fields came first)."""
        d, stepper = self.deferred, self._owed_by
        if d is None:
            return
        self.abandon_deferred()
        try:
            stepper._step(*d)
        except BaseException:
            # not enqueued: the step stays owed (the next use of any of its fields tries again and raises again)
            self._owe(stepper, d)
            raise

    def _room_for_a_third_field(self, stepper, f):
        """After a fused pair one field holds f(t+1) only virtually, and reading it takes a temporary third population field
        (_materialise).  A run whose two fields just fit — the reference's protocol needs no more — must not fail with
        hipErrorOutOfMemory in an innocent read: without room for that field (plus 1/16 slack) the calls are not paired.
        hipMemGetInfo is asked at the first pairing and every 256th afterwards."""
        self._room_calls += 1
        if self._room_ok is None or self._room_calls % 256 == 0:
            info = f.info()
            need = info["plane_stride"] * info["cardinality"] * f.dtype.itemsize
            free, _ = stepper._ctx.mem_info()
            self._room_ok = free >= need + need // 16
        return self._room_ok

    def _materialise(self, stepper, field, bcm, miss, omega, t):
        """`field` should hold f(t+1) but its buffer holds f(t) (a fused pair passed it by): one single step through a
        temporary field, whose buffer the field then adopts.  (Time-dependent walls: t's table is staged again — the ring may
        have moved on since the pair — from the same pure profile.)"""
        # the temporary comes first: if it cannot be allocated this raises with the hook still owed (HookedBuffer.handle puts it
        # back), so the next reader raises again instead of being handed f(t) for f(t+1)
        tmp = stepper._temporary_field()
        try:
            stepper._step(field, tmp, bcm, miss, omega, t)  # (the field carries no hook while its hook runs)
        except BaseException:
            tmp.free()
            raise
        self.n_materialised += 1
        field.exchange_buffers(tmp)
        tmp.free()
