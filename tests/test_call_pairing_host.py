"""The pairing of reference-style calls (xlb_amd/operator/stepper/call_pairing.py) replayed without a device: the real CallPairing, the
real hook rule (_lib.HookedBuffer), the real flusher list (_lib.DeferredWork) and the stepper's own hip_implementation / run / flush_deferred
run on stand-in fields, and a recording stand-in takes the place of the native side (_step, _step2, _step2_eligible, _temporary_field,
the native run loop).  Every sequence of tests/_stepper_sequences.py that goes through the Python layer is applied to it and to the
model's dry run (Sim(..., contents=False)) side by side: the same single steps, fused passes and materialisations, op by op, the same
deferred record, the same lazy state, the same counters.  tests/test_gpu_stepper_sequences.py replays the same table on the device,
with contents.  Below the table: the failure paths that tests/test_gpu_lazy_pairs.py forces on the device, forced here."""

import functools
import gc
import itertools
import weakref

import numpy as np
import pytest

from xlb_amd._lib import DeferredWork, HookedBuffer
from xlb_amd.operator.stepper.call_pairing import CallPairing, is_virtual
from xlb_amd.operator.stepper.nse_stepper import IncompressibleNavierStokesStepper

import _stepper_sequences as sq

SEQS = tuple(q for q in sq.sequences() if not q.setup.native)
CALLS = ("call", "call_noswap", "call_omega", "call_second", "call_gap")


class HostField(HookedBuffer):
    """a field without a device: a token for its buffer, the hook rule of the real one"""

    _tokens = itertools.count(1)

    def __init__(self, halo=0, temporary=False):
        super().__init__(next(self._tokens))
        self.halo, self.temporary, self.dtype = halo, temporary, np.dtype(np.float32)

    buffer = property(lambda self: self._h)  # (raw, as tests/test_gpu_lazy_pairs.py reads it: .handle would count as a use)

    def _release(self):
        if self._h is not None:
            self.released, self._h = self._h, None

    def info(self):
        self.handle
        return {"plane_stride": 12 * 16 * 64, "cardinality": 19}


class HostContext(DeferredWork):
    def mem_info(self):
        return 1 << 30, 1 << 31

    def get_option(self, key):
        return 0

    def sync(self):
        self.flush_deferred()


def use(*objs):
    """what every C-ABI call does with its field arguments: each through .handle, in order"""
    for o in objs:
        if o is not None:
            o.handle


class _NativeLoop:
    """xlbhip_run_any as the Python layer sees it: the fields are used, the result lands where the model says"""

    def __init__(self, stepper):
        self.stepper = stepper

    def run(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        use(f_a, f_b, bc_mask, missing_mask)
        self.stepper.log.append(("run",))
        return self.stepper.result_in_b


class HostStepper(IncompressibleNavierStokesStepper):
    """The stepper's Python layer as it is — hip_implementation, run, flush_deferred, abandon_deferred, the read-only views — on the
    interface CallPairing asks for, which records instead of stepping: ("single" | "pass2", k), ("materialise", field), ("run",)."""

    def __init__(self, ctx, k, log, lazy=True):  # (not the stepper's constructor: no grid, no library)
        self._host_ctx, self.k, self.log = ctx, k, log
        self._pairing = CallPairing(self) if lazy else None
        self.fuses, self.walls_in_time, self.result_in_b = True, False, False
        self.no_memory = self.no_step = False
        self.last_pass, self.adopted = None, []

    _ctx = property(lambda self: self._host_ctx)

    def _step(self, f_src, f_dst, bc_mask, missing_mask, omega, t):
        if self.no_step:
            raise RuntimeError("the step could not be enqueued (simulated)")
        use(f_src, f_dst, bc_mask, missing_mask)
        if f_dst.temporary:
            self.adopted.append((f_dst, f_src.buffer))
        self.log.append(("materialise", f_src) if f_dst.temporary else ("single", self.k))

    def _step2(self, f_src, f_dst, bc_mask, missing_mask, omega, t):
        use(f_src, f_dst, bc_mask, missing_mask)
        self.last_pass = (f_src, f_dst, f_src.buffer, f_dst.buffer)
        self.log.append(("pass2", self.k))

    def _step2_eligible(self, f_src, f_dst, bc_mask, missing_mask):
        use(f_src, f_dst, bc_mask, missing_mask)
        return self.fuses

    def _time_dependent_bcs(self):
        return ["a wall that moves in time"] if self.walls_in_time else []

    def _temporary_field(self):
        if self.no_memory:
            raise MemoryError("hipMalloc failed (simulated)")
        return HostField(temporary=True)

    def _native_stepper(self):
        return _NativeLoop(self)

    def _run_chunked(self, f_0, f_1, bc_mask, missing_mask, omega, n_steps, first_timestep):
        if n_steps:  # (no chunk, no use of the fields)
            use(f_0, f_1, bc_mask, missing_mask)
        self.log.append(("run",))
        return (f_1, f_0) if self.result_in_b else (f_0, f_1)

    def call(self, f_0, f_1, bc_mask, missing_mask, omega, t):
        """one reference-style call; a fused pass must have exchanged the two fields' buffers"""
        self.hip_implementation(f_0, f_1, bc_mask, missing_mask, omega, t)
        if self.last_pass is not None:
            (src, dst, b_src, b_dst), self.last_pass = self.last_pass, None
            assert (src.buffer, dst.buffer) == (b_dst, b_src), "a fused pass without the exchange of buffers"

    def check_adoptions(self):
        """a materialised field has adopted the temporary's buffer: the temporary took the field's old one with it when it was freed"""
        for tmp, old_buffer in self.adopted:
            assert tmp.buffer is None and tmp.released == old_buffer
        self.adopted.clear()


def lazy_state(fields, steppers):
    if any(is_virtual(f) for f in fields):
        return "virtual"
    return "deferred" if any(st._deferred is not None for st in steppers) else "none"


def model_events(sim, i, until_run):
    """the model's events of op i that belong to the Python layer: for a run op those before its marker (the rest is the native loop's)"""
    out = []
    for j, kind, detail in sim.events:
        if j == i and kind == "run" and until_run:
            break
        if j == i and kind in ("single", "pass2", "materialise"):
            out.append((kind, detail if kind == "materialise" else detail["k"]))
    return out


@functools.lru_cache(maxsize=None)
def replay(q):
    """-> the number of (single steps, fused passes, materialisations) this layer made, checked against the model op by op"""
    s = q.setup
    sim = sq.Sim(s, q.seed, contents=False)
    ctx, log = HostContext(), []
    steppers = [HostStepper(ctx, k, log) for k in (0, 1)]
    for st in steppers:
        st.walls_in_time = sq.time_dependent(s)
    new_pop = lambda: HostField(s.halo)  # noqa: E731
    cur, oth, bm, mm, t = new_pop(), new_pop(), HostField(s.halo), HostField(s.halo), 0
    objs = {sim.G.cur: cur, sim.G.oth: oth}  # the model's population ids -> the stand-in fields
    totals = dict(single=0, pass2=0, materialise=0)

    def compare(i, op, until_run=False):
        got = log[: log.index(("run",))] if until_run else list(log)
        want = [(kind, objs[d] if kind == "materialise" else d) for kind, d in model_events(sim, i, until_run)]
        assert got == want, f"op {i} {op}: the layer made {got}, the model {want}"
        for kind, _ in got:
            totals[kind] += 1
        log.clear()
        for st in steppers:
            st.check_adoptions()

    for i, op in enumerate(q.ops):
        kind = op[0]
        for st in steppers:  # step2_eligible answers as the model would have before the op
            st.fuses = sim.fuses()
        exp = sim.apply(op)
        f = {"cur": cur, "oth": oth}.get(op[1]) if len(op) > 1 and isinstance(op[1], str) else None
        if kind in CALLS:
            t += kind == "call_gap"
            steppers[kind == "call_second"].call(cur, oth, bm, mm, sq.OMEGAS[1] if kind == "call_omega" else sq.OMEGAS[0], t)
            if kind != "call_noswap":
                cur, oth, t = oth, cur, t + 1
        elif kind == "run":
            a, b = cur, oth
            steppers[0].result_in_b = exp["result_in_b"]
            cur, oth = steppers[0].run(a, b, bm, mm, sq.OMEGAS[0], op[1], first_timestep=t)
            assert (cur is b) == exp["result_in_b"]
            t += op[1]
        elif kind in ("numpy", "get_plane", "macro", "assign", "set_plane", "fill", "equilibrium", "touch"):
            use(f)
        elif kind == "sync":
            ctx.sync()
        elif kind == "mask_numpy":
            use(bm if op[1] == "bm" else mm)
        elif kind == "copy_from":
            use(oth, cur)
        elif kind == "stream":
            use(cur, oth)
        elif kind == "mask_assign":
            use(bm, mm)
        elif kind == "mask_new":  # freed: what is owed on them runs first
            bm.free()
            mm.free()
            bm, mm = HostField(s.halo), HostField(s.halo)
        elif kind == "fields_new":
            cur.free()
            oth.free()
            cur, oth = new_pop(), new_pop()
        elif kind == "pin":  # __cuda_array_interface__: info(), pinned, ctx.sync()
            f.info()
            f._pinned = True
            ctx.sync()
        elif kind == "plan":
            use(cur, oth, bm, mm)
        elif kind != "option":
            raise ValueError(kind)
        assert objs.setdefault(sim.G.cur, cur) is cur and objs.setdefault(sim.G.oth, oth) is oth, f"op {i} {op}: the fields went another way"
        compare(i, op, until_run=kind == "run")
        for k, st in enumerate(steppers):
            d, real = sim.deferred[k], st._deferred
            assert (d is None) == (real is None), f"op {i} {op}: stepper {k} deferred {real}, the model {d}"
            if d is not None:
                assert real[0] is objs[d["src"]] and real[1] is objs[d["dst"]] and real[2] is bm and real[3] is mm and d["masks"] == sim.G.masks
        assert lazy_state((cur, oth), steppers) == sim.state(), f"op {i} {op}: {lazy_state((cur, oth), steppers)}, the model {sim.state()}"
    # the end, as the device test looks at it: every defined field, then both masks — what is still owed runs now, and counts
    sim.final()
    use(*[fld for fld, name in ((cur, sim.G.cur), (oth, sim.G.oth)) if sim.pops[name] is not None], bm, mm)
    compare(len(q.ops), "final")
    got = [(st._n_fused_pairs, st._n_materialised) for st in steppers]
    assert got == [(sim.n_fused[k], sim.n_materialised[k]) for k in (0, 1)], f"(fused pairs, materialisations) per stepper object: {got}"
    assert totals["pass2"] == sum(sim.n_fused.values()) and totals["materialise"] == sum(sim.n_materialised.values())
    return totals["single"], totals["pass2"], totals["materialise"], sum(kind == "materialise" for _, kind, _ in sim.events), sum(sim.n_fused.values())


@pytest.mark.parametrize("q", SEQS, ids=sq.seq_id)
def test_sequence_on_the_host(q):
    replay(q)


def test_the_whole_table_is_replayed():
    """no skip list: every sequence that goes through the Python layer, and together they make every fused pair and every
    materialisation the model counts (the fused passes inside run() are the native loop's, not this layer's)"""
    assert len(SEQS) == sum(s.n_sequences for s in sq.SETUPS if not s.native) and len(SEQS) >= 100
    singles, passes, materialised, model_materialised, model_pairs = (sum(x) for x in zip(*[replay(q) for q in SEQS]))
    print(f"{len(SEQS)} sequences: {singles} single steps, {passes} fused pairs, {materialised} materialisations")
    assert materialised == model_materialised > 0 and passes == model_pairs > 0 and singles > 0


# ---- the failure paths --------------------------------------------------------------------------------------------------------------
def fresh(lazy=True, n_steppers=1):
    ctx, log = HostContext(), []
    steppers = [HostStepper(ctx, k, log, lazy) for k in range(n_steppers)]
    return ctx, log, steppers, [HostField() for _ in range(4)]


def pair(st, a, b, bm, mm, t=0):
    st.call(a, b, bm, mm, 1.2, t)
    st.call(b, a, bm, mm, 1.2, t + 1)  # fused: b holds f(t+1) virtually
    assert st._n_fused_pairs == 1 and is_virtual(b) and st.log == [("pass2", st.k)]
    st.log.clear()


@pytest.mark.parametrize("first", ["field", "bc_mask", "missing_mask"])
def test_failed_materialisation_keeps_the_step_owed(first):
    """the temporary field cannot be created: the read raises, the next one raises again, the one after succeeds — one materialisation,
    never f(t) for f(t+1); the same when a mask is used first"""
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    pair(st, a, b, bm, mm)
    used = {"field": b, "bc_mask": bm, "missing_mask": mm}[first]
    st.no_memory = True
    for _ in range(2):
        with pytest.raises(MemoryError):
            used.handle
        assert is_virtual(b) and bm.hook is not None and mm.hook is not None and st._n_materialised == 0 and log == []
    st.no_memory = False
    used.handle
    assert log == [("materialise", b)] and st._n_materialised == 1
    st.check_adoptions()
    use(a, b, bm, mm)
    assert len(log) == 1 and all(f.hook is None for f in (a, b, bm, mm))


def test_a_step_that_fails_in_a_flush_stays_owed():
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    st.call(a, b, bm, mm, 1.2, 0)
    record = st._deferred
    assert record[:4] == (a, b, bm, mm) and log == []
    st.no_step = True
    for used in (a, mm, b):
        with pytest.raises(RuntimeError):
            used.handle
        assert st._deferred is record and all(f.hook is not None for f in (a, b, bm, mm))
    with pytest.raises(RuntimeError):
        ctx.sync()
    st.no_step = False
    bm.handle
    assert log == [("single", 0)] and st._deferred is None and all(f.hook is None for f in (a, b, bm, mm))


def test_a_field_abandoned_while_virtual_is_released_at_once():
    """the masks know the field only weakly: no cycle that would wait for the collector, and using them afterwards owes nothing"""
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    pair(st, a, b, bm, mm)
    gone = weakref.ref(b)
    gc.disable()
    try:
        del b
        assert gone() is None
    finally:
        gc.enable()
    use(bm, mm, a)
    assert log == [] and st._n_materialised == 0


def test_the_stepper_is_no_part_of_a_cycle_and_stays_while_a_step_is_owed():
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    st.call(a, b, bm, mm, 1.2, 0)
    gone = weakref.ref(st)
    gc.disable()
    try:
        del st
        assert gone() is not None  # the deferred step needs it
        a.handle
        assert log == [("single", 0)] and gone() is None
    finally:
        gc.enable()
    ctx.sync()  # (its entry in the context's list is forgotten)


def test_a_second_stepper_flushes_the_first_ones_deferred_step():
    ctx, log, (st0, st1), (a, b, bm, mm) = fresh(n_steppers=2)
    st0.call(a, b, bm, mm, 1.2, 0)
    st1.call(b, a, bm, mm, 1.2, 1)  # through the hooks: its own eligibility question uses the fields
    assert log == [("single", 0)] and st0._deferred is None and st1._deferred[:2] == (b, a)
    c, d = HostField(), HostField()
    st0.call(c, d, bm, mm, 1.2, 0)  # the masks are shared: st1's step runs first; then both have one deferred
    assert log == [("single", 0), ("single", 1)] and st0._deferred is not None and st1._deferred is None
    st1.call(a, b, None, None, 1.2, 2)
    log.clear()
    ctx.sync()  # through the context: both
    assert sorted(log) == [("single", 0), ("single", 1)] and st0._deferred is None and st1._deferred is None
    assert all(f.hook is None for f in (a, b, c, d, bm, mm))


def test_abandon_deferred_forgets_the_step():
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    st.call(a, b, bm, mm, 1.2, 0)
    st.abandon_deferred()
    assert st._deferred is None and all(f.hook is None for f in (a, b, bm, mm))
    use(a, b, bm, mm)
    ctx.sync()
    assert log == []


def test_no_pairing_without_room_pinned_or_with_ghost_planes(monkeypatch):
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    asked = []
    monkeypatch.setattr(HostContext, "mem_info", lambda self: asked.append(1) or (1 << 19, 1 << 38))
    for i in range(4):
        st.call(a, b, bm, mm, 1.4, i)
        a, b = b, a
    assert log == [("single", 0)] * 4 and st._n_fused_pairs == 0 and st._deferred is None and len(asked) == 1
    monkeypatch.setattr(HostContext, "mem_info", lambda self: asked.append(1) or (1 << 30, 1 << 38))
    for i in range(4, 260):  # asked again at the 256th call that gets this far: four calls are left, two pairs
        st.call(a, b, bm, mm, 1.4, i)
        a, b = b, a
    assert len(asked) == 2 and st._n_fused_pairs == 2
    use(a, b, bm, mm)
    log.clear()
    a._pinned = True  # exported: its memory must stay put
    st.call(a, b, bm, mm, 1.4, 0)
    slab = [HostField(halo=2) for _ in range(4)]
    st.call(*slab, 1.4, 0)
    assert log == [("single", 0)] * 2 and st._deferred is None


def test_without_pairing_every_call_steps_and_a_virtual_destination_is_dropped():
    ctx, log, (st,), (a, b, bm, mm) = fresh()
    plain = HostStepper(ctx, 1, log, lazy=False)
    pair(st, a, b, bm, mm)
    plain.call(a, b, bm, mm, 1.2, 2)  # overwrites b: nothing to materialise
    assert log == [("single", 1)] and st._n_materialised == 0 and not is_virtual(b)
    assert plain._deferred is None and (plain._n_fused_pairs, plain._n_materialised) == (0, 0)
    plain.flush_deferred()
    plain.abandon_deferred()
