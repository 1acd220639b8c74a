"""The table of tests/_stepper_sequences.py, checked with the oracle alone (no GPU, no xlb_amd): every op class meets every lazy state,
every targeted cache rule really is targeted (the defining op pattern is there), and the table can tell — a mask edit changes the next
field a step wrote, a write changes what it overwrites, a plan option changes the restated plan.  tests/test_gpu_stepper_sequences.py
replays the same sequences on the device."""

import time

import numpy as np
import pytest

import _step2_matrix as m
import _stepper_sequences as sq

SEQS = sq.sequences()
BY_SETUP = {s.name: [q for q in SEQS if q.setup is s] for s in sq.SETUPS}


def dry(q):
    """the restated implementation state along the sequence, without contents: [(op, lazy state the op met)], the model afterwards"""
    sim = sq.Sim(q.setup, q.seed, contents=False)
    met = []
    for op in q.ops:
        met.append((op, sim.state()))
        sim.apply(op)
    sim.final()  # (the last look at the fields counts as well)
    return sim, met


def test_table_shape():
    assert 110 <= len(SEQS) <= 140
    # 10 to 16 ops are drawn; a sequence whose last mask edit has not yet been followed by steps under it and a look at their result gets
    # those ops on top (up to three: call, call, numpy), or that edit could not be told from the masks before it
    assert all(10 <= len(q.ops) <= 19 for q in SEQS)
    assert sum(len(q.ops) > 16 for q in SEQS) <= len(SEQS) // 8
    assert [q.n for q in SEQS] == list(range(len(SEQS))) and len({sq.seq_id(q) for q in SEQS}) == len(SEQS)
    assert {s.name for s in sq.SETUPS} >= {"pairs", "fullway", "slab", "inout", "walls_in_time", "two_grids", "singles"}
    assert sq.sequences() is SEQS  # (seeded: the same table every time)
    assert tuple(q.ops for q in sq.sequences.__wrapped__()) == tuple(q.ops for q in SEQS)


@pytest.mark.parametrize("name", ["pairs", "fullway"])
def test_every_op_class_meets_every_lazy_state(name):
    cells = {}
    for q in BY_SETUP[name]:
        for op, state in dry(q)[1]:
            cells[(state, sq.OP_CLASS[op[0]])] = cells.get((state, sq.OP_CLASS[op[0]]), 0) + 1
    missing = [(st, c) for st in sq.STATES for c in ("calls", "reads", "writes", "masks", "fields", "options", "plan") if not cells.get((st, c))]
    assert not missing, f"{name}: no op of these (lazy state, class) cells: {missing}"
    # and every kind of op of the table at least once in the set-up
    kinds = {op[0] for q in BY_SETUP[name] for op in q.ops}
    assert kinds >= set(sq.OP_CLASS) - {"grid", "call_gap"}, sorted(set(sq.OP_CLASS) - {"grid", "call_gap"} - kinds)


def test_the_other_setups_use_their_ops():
    assert {op[0] for q in BY_SETUP["slab"] for op in q.ops}.isdisjoint({"call", "call_noswap", "call_omega", "call_second"})
    assert {("option", "overlap", 0), ("option", "overlap", 1)} & {op for q in BY_SETUP["slab"] for op in q.ops}
    for name in ("two_grids", "two_channels"):
        grids = {op[1] for q in BY_SETUP[name] for op in q.ops if op[0] == "grid"}
        assert grids == set(range(len(BY_SETUP[name][0].setup.grids)))
    # the control never defers and never fuses
    for q in BY_SETUP["singles"]:
        sim, met = dry(q)
        assert {st for _, st in met} == {"none"} and not any(e[1] == "pass2" for e in sim.events)
    # run(n) for n in 0 .. 5
    assert {op[1] for q in SEQS for op in q.ops if op[0] == "run" and op[1] <= sq.RING_SLOTS} == set(range(6))
    # call ops on consecutive and non-consecutive timesteps where the walls move in time
    refused = 0  # a call with the fields swapped that meets a deferred step of the timestep before the last: no pair (pairs_in_time)
    for q in BY_SETUP["walls_in_time"]:
        sim = sq.Sim(q.setup, q.seed, contents=False)
        for op in q.ops:
            d, fused = sim.deferred[0], sim.n_fused[0]
            swapped = d is not None and (d["src"], d["dst"], d["masks"]) == (sim.G.oth, sim.G.cur, sim.G.masks)
            sim.apply(op)
            refused += op[0] == "call_gap" and swapped and sim.n_fused[0] == fused and sim.deferred[0] is not None
    assert refused >= 3, refused
    assert any(op[0] == "call" for q in BY_SETUP["walls_in_time"] for op in q.ops)


def _passes(sim):
    return [(i, d) for i, kind, d in sim.events if kind == "pass2"]


def _flags(q, d):
    return [tuple(f) for _, f in sq.restated_plan(q.setup, d["g"], d["variant"], d["options"], False)]


def _tile_counts(q, g):
    tile = m.step2_tile(q.setup.lattice)
    return q.setup.grids[g][1] // tile[0], q.setup.grids[g][2] // tile[1]


def pattern_present(q, rule):
    """the op pattern that defines the rule's tag, on the restated run of the sequence"""
    sim, met = dry(q)
    passes = _passes(sim)
    pairs = list(zip(passes, passes[1:]))
    if rule == "meta":  # two fused passes of one stepper on one grid, the masks edited (contents or objects) in between
        return any(a["k"] == b["k"] and a["g"] == b["g"] and (a["variant"], a["masks"]) != (b["variant"], b["masks"]) for (_, a), (_, b) in pairs)
    if rule == "tile_order":  # consecutive fused passes of one stepper on tilings of different counts
        return any(a["k"] == b["k"] and _tile_counts(q, a["g"]) != _tile_counts(q, b["g"]) for (_, a), (_, b) in pairs)
    if rule == "clean":  # consecutive fused passes whose restated clean flags differ, by the masks and by the launch geometry
        by_masks = any(a["options"] == b["options"] and _flags(q, a) != _flags(q, b) for (_, a), (_, b) in pairs)
        by_plan = any(a["variant"] == b["variant"] and _flags(q, a) != _flags(q, b) for (_, a), (_, b) in pairs)
        return by_masks and by_plan and any(1 in f and 0 in f for _, d in passes for f in _flags(q, d))
    if rule == "scan":  # fused, then single steps because an edge-kind cell sits inside (fuse2 still 2), then fused again
        marks = [(i, "2") for i, _ in passes] + [(i, "1") for i, kind, d in sim.events if kind == "single" and not d["fuses"] and d["fuse2"] == 2
                                                 and any(op == ("mask_assign", "inlet_in") for op in q.ops[:i])]
        return "212" in "".join(c for _, c in sorted(marks)).replace("22", "2").replace("11", "1")
    if rule == "scratch":  # the channel's stepper: fused passes on fields of different shapes, there and back
        gs = [d["g"] for _, d in passes]
        return q.setup.background == "inout" and any(gs[i] != gs[i + 1] and gs[i] in gs[i + 2 :] for i in range(len(gs) - 2))
    if rule == "strips":  # a fused pass whose source carries the strips of earlier contents
        return any(d["stale_src"] and not d["strips_read"] for _, d in passes)
    if rule == "profile_ring":  # a run that stages more tables than the ring holds, then a fused pair of calls whose virtual field is read
        long_runs = [i for i, kind, d in sim.events if kind == "run" and d["n"] > sq.RING_SLOTS]
        fused = [i for i, d in passes if long_runs and i > long_runs[0] and q.ops[i][0] == "call"]
        return sq.time_dependent(q.setup) and bool(fused) and any(i > fused[0] for i, kind, _ in sim.events if kind == "materialise")
    if rule == "virtual_masks":  # a mask edit that meets a virtual field (and so materialises it)
        return any(sq.OP_CLASS[op[0]] == "masks" and st == "virtual" and (i, "materialise") in {(e[0], e[1]) for e in sim.events} for i, (op, st) in enumerate(met))
    raise ValueError(rule)


def test_every_rule_is_hit_by_two_sequences():
    for rule in sq.RULES:
        tagged = [q for q in SEQS if rule in q.tags]
        assert len(tagged) >= 2, rule
        absent = [sq.seq_id(q) for q in tagged if not pattern_present(q, rule)]
        assert not absent, f"tagged {rule} without its pattern: {absent}"
    # the strips rule also has to be met with valid strips (a pass that READS them), or a mutant that never reads them would pass
    assert sum(any(d["strips_read"] for _, d in _passes(dry(q)[0])) for q in SEQS) >= 10


def test_counts_predicted():
    fused = [q for q in SEQS if sum(dry(q)[0].n_fused.values()) > 0]
    materialised = [q for q in SEQS if sum(dry(q)[0].n_materialised.values()) > 0]
    assert 3 * len(fused) >= len(SEQS), len(fused)
    assert len(materialised) >= 10, len(materialised)


def test_the_second_stepper_object_takes_part():
    """a call through the second object meets a deferred step of the first and flushes it; the second object defers, fuses a pair and
    materialises its virtual field — each in at least three sequences, read off the restated run"""
    flushes_first, defers, fuses, materialises = set(), set(), set(), set()
    for q in SEQS:
        sim = sq.Sim(q.setup, q.seed, contents=False)
        for i, op in enumerate(q.ops):
            first = sim.deferred[0]
            sim.apply(op)
            if op[0] == "call_second":
                if first is not None and sim.deferred[0] is None and any(e[0] == i and e[1] == "single" and e[2]["k"] == 0 for e in sim.events):
                    flushes_first.add(q.n)
                if sim.deferred[1] is not None:
                    defers.add(q.n)
        sim.final()
        if sim.n_fused[1]:
            fuses.add(q.n)
        if sim.n_materialised[1]:
            materialises.add(q.n)
    assert min(len(flushes_first), len(defers), len(fuses), len(materialises)) >= 3, (flushes_first, defers, fuses, materialises)
    assert {q.n for q in SEQS if "second_stepper" in q.tags} <= flushes_first & defers & fuses & materialises


ORACLE_SECONDS = {}


@pytest.mark.parametrize("name", [s.name for s in sq.SETUPS])
def test_table_discriminates(name):
    """without exception: every mask edit changes the next observed field that a later step wrote, every write changes what it overwrites,
    every plan option changes the restated plan.  (The oracle's time for the whole table: about half a minute, printed with -s.)"""
    t0 = time.perf_counter()
    bad = [(sq.seq_id(q), sq.discrimination_failures(q)) for q in BY_SETUP[name]]
    bad = [b for b in bad if b[1]]
    ORACLE_SECONDS[name] = time.perf_counter() - t0
    print(f"oracle time {name}: {ORACLE_SECONDS[name]:.1f} s; table so far {sum(ORACLE_SECONDS.values()):.1f} s")
    assert not bad, bad


@pytest.mark.parametrize("q", [q for q in SEQS if "virtual_masks" in q.tags], ids=sq.seq_id)
def test_an_edited_mask_would_change_the_virtual_field(q):
    """the situation the tag is about: a field holds f(t+1) virtually, the masks are edited, the field is read.  The model keeps the step
    with the masks of the call; a stepper that materialised with the edited masks would give another field (so the device test can tell)."""
    sim = sq.Sim(q.setup, q.seed)
    for i, op in enumerate(q.ops):
        if sq.OP_CLASS[op[0]] == "masks" and sim.state() == "virtual":
            v = next(h[2] for h in sim.hooks.values() if h[0] == "mat")
            base, omega, t = sim.base[v]
            owed = sim.pops[v]
            assert np.array_equal(owed, sq._step(q.setup, sim.g, sim.G.variant, omega, base, t))
            assert not np.array_equal(owed, sq._step(q.setup, sim.g, op[1], omega, base, t)), "the edited masks give the same f(t+1)"
            assert q.ops[i + 1] == ("numpy", "oth") and getattr(sim.G, "oth") == v
            return
        sim.apply(op)
    raise AssertionError("no mask edit met a virtual field")


def test_inlet_variant_keeps_the_oracle_finite():
    """the channel's interior inlet cell: the single-step path runs there, and the comparison is bit for bit — no NaN may come out of it"""
    for q in BY_SETUP["inout"] + BY_SETUP["two_channels"]:
        sim, seen = sq.replay(q)
        for fin in sim.final():
            assert all(fin[slot] is None or np.isfinite(fin[slot]).all() for slot in ("cur", "oth")), sq.seq_id(q)
