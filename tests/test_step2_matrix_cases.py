"""The conditions the case table of the two-step kernel's sweep (tests/_step2_matrix.py) must meet, checked with the restated plan and
the oracle alone (no GPU): what makes a case worth running is decided here, not by what the kernel does with it.  The conditions
are caps, not measurements: an input that cannot meet one is changed in the generator."""

import collections

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _step2_matrix as m

CASES = m.cases()


def test_expected_table_size():
    """313 cases, 731 GPU runs with the knob sets (a third of the table under each alternative), 31 reference-protocol runs.  A change
    of the generator that moves these numbers is meant to be seen here."""
    assert len(CASES) == 313
    assert sum(len(m.knob_sets(c)) for c in CASES) == 731
    assert sum(m.runs_reference_protocol(c) for c in CASES) == 31
    per_knob = collections.Counter(k.name for c in CASES for k in m.knob_sets(c))
    assert per_knob["default"] == len(CASES) and all(abs(per_knob[k.name] - len(CASES) / 3) <= 1 for k in m.KNOBS[1:])


def test_ids_are_unique_and_steppers_stay_within_the_fast_bc_slots():
    ids = [m.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        specs = m.bc_specs(c.setup, c.background, c.probe, c.pos)
        assert 1 <= len(specs) <= 8 and [s.id for s in specs] == list(range(1, len(specs) + 1))
        assert all(0 <= v < n for v, n in zip(c.pos, c.setup.shape))
        assert c.steps in m.STEPS and c.omega in m.OMEGAS


def test_boxes_are_the_smallest_of_their_path():
    """the plan each set-up was chosen for"""
    plan = {s.name: [(l.x_begin, l.x_count, l.segments, l.cap) for l in m.default_launches(s)] for s in m.SETUPS}
    assert plan["x4"] == [(0, 32, 4, 8)] and plan["x3"] == [(0, 24, 3, 8)]
    assert plan["slab_overlap"] == [(2, 28, 3, 8), (0, 2, 1, 0), (30, 2, 1, 0)] and plan["slab_whole"] == [(0, 32, 3, 8)]
    assert plan["auto4"] == [(0, 128, 4, 8)] and plan["auto2"] == [(0, 64, 2, 0)]
    assert plan["q27"] == [(0, 24, 3, 8)] and plan["inout"] == [(2, 28, 3, 8)]
    by = {s.name: s for s in m.SETUPS}
    assert [it[1:] for it in m.default_launches(by["x4"])[0].items[::4]] == [(0, 8), (8, 16), (16, 24), (24, 32)]
    assert [it[1:] for it in m.default_launches(by["auto4"])[0].items] == [(0, 8), (8, 64), (64, 120), (120, 128)]
    assert m.default_launches(by["q27"])[0].tile == (8, 48) and m.default_launches(by["q27"])[0].shift == (4, 24)
    assert max(s.shape for s in m.SETUPS) <= (128, 8, 64) and all(np.prod(s.shape) <= 64 * 16 * 128 for s in m.SETUPS)
    # without clean items the caps go and the automatic rule keeps its segments
    assert [it[1:] for it in m.pass_launches("D3Q19", (128, 8, 64), 0, 1, 0, m.KNOBS[1], False)[0].items] == [(0, 32), (32, 64), (64, 96), (96, 128)]


def test_every_probe_kind_meets_every_position_class_on_the_bare_background():
    seen = collections.defaultdict(set)
    for c in CASES:
        if c.background == "bare":
            for axis in range(3):
                seen[(axis, c.probe)].add(c.classes[axis])
    for probe in m.PROBES:
        assert seen[(0, probe)] >= set(m.X_TYPES), (probe, seen[(0, probe)])
        for axis in (1, 2):
            assert seen[(axis, probe)] >= set(m.YZ_TYPES), (axis, probe, seen[(axis, probe)])
    for background in ("plates", "cavity_hw", "cavity_fw"):
        z = {c.classes[2] for c in CASES if c.background == background}
        assert z >= set(m.WALL_Z_TYPES), (background, z)
        assert any(c.role == ("yz_edge",) for c in CASES if c.background == background)
    # a one-index halfway solid given by an interior index tags its footprint (19 cells, 27 on D3Q27), a single-cell probe one cell
    for c in CASES:
        if c.background == "bare" and c.classes == ("interior",) * 3:
            n = int((m.case_masks(c).bc_mask != 0).sum())
            assert n == {"fw": 1, "eq": 1, "hw": m.case_masks(c).lat.q, "hwm": m.case_masks(c).lat.q}.get(c.probe, n)


def _sweep(setup):
    return {c.role[1:]: c for c in CASES if c.setup is setup and c.role[0] == "sweep"}


def _boundaries(setup):
    """(axis, instance, side, rim offset, offset one further out): both sides of every seam and of every segment boundary"""
    out = []
    for axis in range(3):
        if axis > 0 and setup.shape[axis] == m.step2_tile(setup.lattice)[axis - 1]:
            continue
        n = len(m.segment_starts(setup) if axis == 0 else m.seams(setup, axis))
        for i in range(n):
            out.append((axis, i, "lo", -1, -2))  # the item that starts at the boundary
            out.append((axis, i, "hi", 0, 2 if axis == 0 else 1))  # the item that ends there
    return out


@pytest.mark.parametrize("setup", [s for s in m.SETUPS if not s.inout], ids=lambda s: s.name)
def test_rim_probes_and_their_clean_neighbours(setup):
    """For every seam and segment boundary of the set-up's plan and either side of it: a case whose probe lies in the rim of the item on
    that side (grown tile minus tile; plane x_lo - 1 or x_hi) and in none of its own cells, so that the item is dirty because of the rim
    alone — and the probe changes a population INSIDE the item after two oracle steps, so a flag wrongly 1 gives wrong numbers —
    next to the case one class further out, whose probe leaves that item clean."""
    shape, slab = setup.shape, setup.halo > 0
    sweep = _sweep(setup)
    bounds = _boundaries(setup)
    assert len(sweep) == 2 * len(bounds) and len(bounds) >= 8
    for axis, i, side, rim_off, far_off in bounds:
        rim, far = sweep[(axis, i, rim_off)], sweep[(axis, i, far_off)]
        b = (m.segment_starts(setup) if axis == 0 else m.seams(setup, axis))[i]
        assert rim.pos[axis] == (b + rim_off) % shape[axis] and far.pos[axis] == (b + far_off) % shape[axis]
        assert all(rim.pos[a] == far.pos[a] for a in range(3) if a != axis) and rim.probe in ("fw", "eq") and far.probe in ("fw", "eq")
        tagged = m.case_masks(rim).bc_mask[0] != 0
        assert tagged.sum() == 1 and tagged[rim.pos]
        found = []
        for (launch, flags), (launch_far, flags_far) in zip(m.restated_plan(rim), m.restated_plan(far)):
            assert launch == launch_far and launch.has_flags
            for k, item in enumerate(launch.items):
                (gx, gy, gz), (px, py, pz) = m.item_cells(launch, item, shape, slab)
                in_grown = rim.pos[0] in gx and rim.pos[1] in gy and rim.pos[2] in gz
                in_own = rim.pos[0] in px and rim.pos[1] in py and rim.pos[2] in pz
                assert flags[k] == (0 if in_grown else 1)
                ty0 = (item[0] // (shape[2] // launch.tile[1])) * launch.tile[0] + launch.shift[0]
                tz0 = (item[0] % (shape[2] // launch.tile[1])) * launch.tile[1] + launch.shift[1]
                start = (item[1], ty0, tz0)[axis] % shape[axis]
                end = (item[2], ty0 + launch.tile[0], tz0 + launch.tile[1])[axis] % shape[axis]
                if in_grown and not in_own and (start if side == "lo" else end) == b % shape[axis]:
                    found.append((launch, item, flags_far[k]))
        assert found, (m.case_id(rim), side)
        with_probe, without = m.expected(rim, steps=2), m.expected(rim, steps=2, probe=False)
        assert np.isfinite(with_probe).all()
        hit = False
        for launch, item, far_flag in found:
            assert far_flag == 1, (m.case_id(far), item)
            _, (px, py, pz) = m.item_cells(launch, item, shape, slab)
            own = np.ix_(range(with_probe.shape[0]), px, py, pz)
            hit |= bool((with_probe[own] != without[own]).any())
        assert hit, f"{m.case_id(rim)}: the probe changes nothing inside the item it dirties"


def test_every_case_keeps_clean_and_dirty_items():
    """With fuse2_clean and a launch of three or more segments, the items of the pass that read flags hold a clean and a dirty one:
    no such case leaves the BC-free body or the hull body unexercised.  (The inlet / outlet middle launch reads no flags: all its
    items are 0; so are all items without fuse2_clean.)"""
    n = 0
    for c in CASES:
        assert m.keeps_clean_and_dirty_items(c), m.case_id(c)
        n += any(l.has_flags and l.segments >= 3 for l, _ in m.restated_plan(c))
        if c.setup.inout:
            assert all(f == 0 for _, flags in m.restated_plan(c) for f in flags)
        for knobs in m.KNOBS[1:2]:
            assert all(f == 0 for _, flags in m.restated_plan(c, knobs) for f in flags)
    assert n >= 250


def _neighbour_axes(launch, flags, shape):
    """per clean item of a launch, the axes along which an adjacent item (next segment of its tile column; next tile row / column of
    its segment, periodically) is dirty"""
    tys, tzs = shape[1] // launch.tile[0], shape[2] // launch.tile[1]
    by = {}
    for k, (t, lo, hi) in enumerate(launch.items):
        by[(t // tzs, t % tzs, lo)] = (flags[k], hi)
    out = []
    for (ty, tz, lo), (flag, hi) in by.items():
        if flag != 1:
            continue
        axes = set()
        for (ty2, tz2, lo2), (flag2, hi2) in by.items():
            if flag2 != 0:
                continue
            if (ty2, tz2) == (ty, tz) and (lo2 == hi or hi2 == lo):
                axes.add(0)
            if lo2 == lo and tz2 == tz and ty2 != ty and (ty2 - ty) % tys in (1, tys - 1):
                axes.add(1)
            if lo2 == lo and ty2 == ty and tz2 != tz and (tz2 - tz) % tzs in (1, tzs - 1):
                axes.add(2)
        out.append(axes)
    return out


def test_clean_items_lie_next_to_dirty_ones_along_every_axis():
    """Every background has, for each of x, y and z, a case in which a clean item is adjacent to a dirty one along that axis; on the
    cavities one clean item has dirty neighbours along all three at once (one probe on a periodic background cannot dirty the three
    neighbours of an item without touching the item)."""
    seen, all_three = collections.defaultdict(set), set()
    for c in CASES:
        for launch, flags in m.restated_plan(c):
            if launch.has_flags:
                for axes in _neighbour_axes(launch, flags, c.setup.shape):
                    seen[c.background] |= axes
                    if axes == {0, 1, 2}:
                        all_three.add(c.background)
    for background in ("bare", "plates", "cavity_hw", "cavity_fw"):
        assert seen[background] == {0, 1, 2}, (background, seen[background])
    assert all_three >= {"cavity_hw", "cavity_fw"}


def _leaving_lanes(c):
    """(nx, ny) lanes per z row of the z-face tile column (the wrap-around one: it holds z = 0 and z = nz - 1) that are halfway-wall
    cells whose missing set lies in neither c_z sign set — the lanes that take a row wave out of the face arm (step2_kernel.hpp: bc_arm)"""
    ms = m.case_masks(c)
    lat, shape = ms.lat, c.setup.shape
    halfway = [s.id for s in m.bc_specs(c.setup, c.background, c.probe, c.pos) if s.kind == orc.KIND_HALFWAY_BB]
    bits = (ms.missing_mask.astype(np.uint32) << np.arange(lat.q, dtype=np.uint32).reshape(-1, 1, 1, 1)).sum(axis=0)
    bits = np.where(np.isin(ms.bc_mask[0], halfway), bits, 0)
    czp = sum(1 << l for l in range(lat.q) if lat.c[2, l] == 1)
    czm = sum(1 << l for l in range(lat.q) if lat.c[2, l] == -1)
    leaves = ((bits & ~np.uint32(czp)) != 0) & ((bits & ~np.uint32(czm)) != 0)
    tz, oz = m.step2_tile(c.setup.lattice)[1], m.tile_shift(m.step2_tile(c.setup.lattice))[1]
    zs = [(shape[2] - tz + oz + i) % shape[2] for i in range(tz)]
    assert 0 in zs and shape[2] - 1 in zs
    return leaves[:, :, zs].sum(axis=2)


@pytest.mark.parametrize("background", ["plates", "cavity_hw"])
def test_a_lane_takes_its_z_face_row_out_of_the_face_arm(background):
    """A halfway solid touching the wall z = 0 gives its diagonal neighbours (x +- 1, y +- 1, z = 1) an x-y missing bit: the z-face row
    through such a cell holds exactly ONE lane whose missing set leaves the c_z sign sets, and the rows around it none; in another
    case of the same set-up and background that row holds none."""
    arms = [c for c in CASES if c.background == background and c.role == ("arm",) and c.setup.lattice == "D3Q19"]
    assert arms
    for c in arms:
        lanes = _leaving_lanes(c)
        row = (c.pos[0] + 1, c.pos[1] + 1)
        assert lanes[row] == 1 and lanes[row[0] + 1, row[1]] == 0 and lanes[row[0], row[1] + 1] == 0
        others = [o for o in CASES if o.setup is c.setup and o.background == background and o is not c]
        assert any(_leaving_lanes(o)[row] == 0 for o in others)


def test_every_oracle_run_stays_finite():
    for c in CASES:
        out = m.expected(c)
        assert out.dtype == np.float32 and np.isfinite(out).all(), m.case_id(c)
        assert not np.array_equal(out, m.f_init(c))
