"""The case matrix of the two-steps-per-pass kernel k_step2 (csrc/step2_kernel.hpp) and the launch plan of a pass, restated.  No GPU and
no xlb_amd here: tests/test_step2_matrix_cases.py checks the generator with the oracle alone, and tests/test_gpu_step2_matrix.py
builds the matching xlb_amd objects from the same records and compares the device's plan report (xlbhip_step2_plan) with the
restatement, and the populations with the oracle.

A case is a box set-up (SETUPS: shape, lattice, ghost planes, fuse2_xseg), a background (bare periodic, halfway plates on the z
faces, halfway or fullway cavity; the inlet / outlet channel has its own), and ONE probe: a small boundary condition placed relative
to the restated plan — next to a tile seam of the half-tile-shifted tiling, next to an x-segment boundary, on the box wrap, inside a
tile.  The probe decides which work items (tile column x x segment) are dirty; clean items run the body without boundary conditions,
so a wrongly clean flag gives wrong numbers and nothing else.

Table (cases()):
  sweep     bare background, one axis at a time with the other two inside an item: for every tile seam s of y and z the coordinates
            s - 2, s - 1, s, s + 1, for every segment start x_lo of every launch x_lo - 2, x_lo - 1, x_lo, x_lo + 2; single-cell probes
            (fullway, equilibrium) in turn.  s - 1 / s and x_lo - 1 / x_lo sit in the rim of the item across the boundary (grown tile
            minus tile, planes x_lo - 1 and x_hi), their neighbours one further out leave that item clean.
  rotation  bare background, every probe kind x every class type of every axis (the offsets above and x_lo + 1, the box wrap, a
            tile-interior coordinate), the three axes paired by rotation and dealt over the set-ups.
  walls     the other backgrounds: per set-up and background a rotating subset of the classes, z also next to the wall lanes
            (1, 2, nz - 3, nz - 2), a halfway solid touching the z wall (role "arm": one lane of a z-face row gains x / y bits) and a
            position next to a y-z edge.
Every case runs with the default options; a rotating third also under each alternative knob set (KNOBS)."""

import functools
from collections import namedtuple

import numpy as np

from oracle import xlb_numpy as orc

# ---- the plan, restated ------------------------------------------------------------------------------------------------------------
CUS = 256  # MI355X; at the boxes of this table the automatic rule gives the same segments for any chip of 32 CUs or more


def step2_tile(lattice, collision="BGK", has_bc=True):
    """step2_plan.hpp:37 step2_tile"""
    return (8, 48 if lattice == "D3Q27" and (collision == "KBC" or has_bc) else 64)


def tile_shift(tile, has_bc=True):
    """stepper.hip:187 make_launch2: half a tile with boundary conditions"""
    return (tile[0] // 2, tile[1] // 2) if has_bc else (0, 0)


def step2_segments(x_count, tiles, xseg, clean, needs_missing, has_bc=True, cus=CUS):
    """step2_plan.hpp:66 step2_segments"""
    if xseg > 0:
        n = xseg
        while n > 1 and x_count // n < 8:
            n //= 2
        return n
    finest = needs_missing or (has_bc and clean)
    best, best_cost, n = 1, -1, 1
    while n <= 8:
        if n > 1 and x_count // n < 32:
            break
        cost = ((tiles * n + cus - 1) // cus) * (x_count // n + 3)
        if best_cost < 0 or cost < best_cost or finest:
            best, best_cost = n, cost
        n *= 2
    return best


def step2_eff_segments(x_segments, x_count):
    """step2_launch.hpp:10 step2_eff_segments"""
    return x_segments if (x_segments > 1 and x_count >= 8 * x_segments) else 1


def step2_eff_cap(x_cap, x_segments, x_count):
    """step2_launch.hpp:12 step2_eff_cap"""
    n = step2_eff_segments(x_segments, x_count)
    return x_cap if (x_cap > 0 and n >= 3 and x_count - 2 * x_cap >= 8 * (n - 2)) else 0


def step2_seg_range(x_begin, x_count, n_seg, x_cap, seg):
    """step2_kernel.hpp:190 step2_seg_range"""
    if x_cap > 0 and n_seg >= 3:
        inner, m = x_count - 2 * x_cap, n_seg - 2
        x_lo = x_begin if seg == 0 else x_begin + x_cap + (inner * (seg - 1)) // m
        x_hi = x_begin + x_cap if seg == 0 else (x_begin + x_count if seg == n_seg - 1 else x_begin + x_cap + (inner * seg) // m)
        if seg == n_seg - 1:
            x_lo = x_begin + x_count - x_cap
        return x_lo, x_hi
    return x_begin + (x_count * seg) // n_seg, x_begin + (x_count * (seg + 1)) // n_seg


def step2_tile_order(tys, tzs):
    """step2_plan.hpp:122 step2_tile_order"""
    hull = [(tys - 1) * tzs + tz for tz in range(tzs)] + [ty * tzs + tzs - 1 for ty in range(tys - 2, -1, -1)]
    inner = [ty * tzs + tz for ty in range(tys - 1) for tz in range(tzs - 1)]
    order = []

    def deal(lst):
        n = len(lst)
        per = (n + 7) // 8
        cur = [min(n, k * per) for k in range(8)]
        end = [min(n, (k + 1) * per) for k in range(8)]
        for _ in range(n):
            k = len(order) % 8
            if cur[k] == end[k]:
                for m in range(8):
                    if end[m] - cur[m] > end[k] - cur[k]:
                        k = m
            order.append(lst[cur[k]])
            cur[k] += 1

    deal(hull)
    deal(inner)
    return order


def block_tile(slot, n_tiles, order, swizzle):
    """step2_kernel.hpp:262 (k_step2) and :732 (k_step2_clean): the tile of block slot `slot` of a segment"""
    if order is not None:
        return order[slot]
    if swizzle:
        per_xcd = n_tiles // 8
        return (slot % 8) * per_xcd + slot // 8
    return slot


Knobs = namedtuple("Knobs", "name clean strips rowmap")
KNOBS = (Knobs("default", 1, 1, 0), Knobs("noclean", 0, 1, 0), Knobs("strips0", 1, 0, 0), Knobs("strips2", 1, 2, 0), Knobs("rowmap", 1, 0, 1))
STRIPS_NONE, STRIPS_WRITE, STRIPS_READ_WRITE, STRIPS_ROWMAP = 0, 2, 3, 4  # step_launch.hpp:45 enum Strips

Launch = namedtuple("Launch", "x_begin x_count segments cap tile shift strips has_flags items")  # items: ((tile, x_lo, x_hi), ...)


def pass_launches(lattice, shape, halo, overlap, xseg, knobs, needs_missing, edge_ext=False, strips_valid=False):
    """The two-step launches of one pass of a stepper WITH boundary conditions (stepper.hip: make_launch2:172, step_twice:330,
    step_twice_edge_ext:249, slab_pass:302, launch_step2:210), in launch order.  strips_valid: the source field carries the strips of
    its current contents (it was written by a strip-writing pass)."""
    nx, ny, nz = shape
    clean_on = knobs.clean != 0
    tile = step2_tile(lattice)
    shift = tile_shift(tile)
    tys, tzs = ny // tile[0], nz // tile[1]
    n_tiles = tys * tzs
    order = step2_tile_order(tys, tzs) if (needs_missing or clean_on) else None  # make_launch2:181
    swizzle = n_tiles % 8 == 0  # step2_launch.hpp:16 step2_eff_swizzle (make_launch2 asks for it)
    x_cap = 8 if clean_on else 0  # make_launch2:183
    d3q19 = lattice == "D3Q19" and tile == (8, 64)
    strips = (knobs.strips == 2 or knobs.strips == 1) and d3q19 and nx >= 8  # step_twice:345 (has_bc)
    rowmap = (not strips) and knobs.rowmap != 0 and d3q19  # step_twice:356

    def launch(x_begin, x_count, role):
        segs = 1 if role == "edge" else step2_segments(x_count, n_tiles, xseg, clean_on, needs_missing)
        n, cap = step2_eff_segments(segs, x_count), step2_eff_cap(x_cap, segs, x_count)
        if role == "middle":
            mode = STRIPS_NONE
        elif strips:
            mode = STRIPS_READ_WRITE if (strips_valid and role in ("all", "interior")) else STRIPS_WRITE
        else:
            mode = STRIPS_ROWMAP if rowmap else STRIPS_NONE
        items = tuple((block_tile(b % n_tiles, n_tiles, order, swizzle),) + step2_seg_range(x_begin, x_count, n, cap, b // n_tiles) for b in range(n_tiles * n))
        return Launch(x_begin, x_count, n, cap, tile, shift, mode, clean_on and role != "middle", items)

    if edge_ext:
        return [launch(2, nx - 4, "middle")]
    if halo == 0:
        return [launch(0, nx, "all")]
    if not (overlap and nx >= 16):
        return [launch(0, nx, "whole")]
    return [launch(2, nx - 4, "interior"), launch(0, 2, "edge"), launch(nx - 2, 2, "edge")]


def item_cells(launch, item, shape, slab):
    """(planes, ys, zs) the clean rule of k_step2_clean (step2_kernel.hpp:745) visits for an item, and the item's own (proper) ones"""
    nx, ny, nz = shape
    (ty, tz), (oy, oz) = launch.tile, launch.shift
    t, x_lo, x_hi = item
    tzs = nz // tz
    ty0, tz0 = (t // tzs) * ty + oy, (t % tzs) * tz + oz
    planes = [(min(p, x_hi) if slab else p) % nx for p in range(x_lo - 1, x_hi + 2)]
    grown = (planes, [(ty0 - 1 + i) % ny for i in range(ty + 2)], [(tz0 - 1 + i) % nz for i in range(tz + 2)])
    proper = ([p % nx for p in range(x_lo, x_hi)], [(ty0 + i) % ny for i in range(ty)], [(tz0 + i) % nz for i in range(tz)])
    return grown, proper


def clean_flags(tagged, launch, slab):
    """k_step2_clean restated on a (nx, ny, nz) bool array of tagged cells (bc_mask != 0: every tagged cell has a non-zero meta word,
    ops_kernels.hpp:938 k_build_meta).  SLAB: the plane x_hi + 1 is clamped to x_hi, and the ghost planes -1 and nx hold the meta words
    of the planes nx - 1 and 0 (one rank: the ring exchange is the periodic wrap)."""
    if not launch.has_flags:
        return [0] * len(launch.items)
    out = []
    for item in launch.items:
        (px, ys, zs), _ = item_cells(launch, item, tagged.shape, slab)
        out.append(0 if tagged[np.ix_(px, ys, zs)].any() else 1)
    return out


# ---- set-ups, backgrounds, probes ----------------------------------------------------------------------------------------------------
Setup = namedtuple("Setup", "name lattice shape halo overlap xseg inout backgrounds")
_ALL_BG = ("bare", "plates", "cavity_hw", "cavity_fw")
SETUPS = (
    Setup("x4", "D3Q19", (32, 16, 128), 0, 1, 4, False, _ALL_BG),  # two inner 8-plane segments between two caps, 2 x 2 tiles
    Setup("x3", "D3Q19", (24, 16, 128), 0, 1, 3, False, _ALL_BG),  # one inner segment
    Setup("slab_overlap", "D3Q19", (32, 16, 128), 2, 1, 3, False, _ALL_BG),  # interior launch [2, 30) in three segments + two edge launches
    Setup("slab_whole", "D3Q19", (32, 16, 128), 2, 0, 3, False, _ALL_BG),
    # one tile that is its own wrap-around row and column: walls on y or z would leave no clean item, so the bare background only
    Setup("auto4", "D3Q19", (128, 8, 64), 0, 1, 0, False, ("bare",)),
    Setup("auto2", "D3Q19", (64, 16, 128), 0, 1, 0, False, _ALL_BG),  # 2 segments, no caps
    Setup("q27", "D3Q27", (24, 16, 96), 0, 1, 3, False, _ALL_BG),  # (8 x 48) tiles, shift (4, 24), wide meta word, generic arm only
    Setup("inout", "D3Q19", (32, 16, 128), 0, 1, 3, True, ("inout",)),  # the middle launch starts at x = 2
)
PROBES = ("fw", "eq", "hw", "hwm", "hw2x", "hw2z")
U_PROBE = (0.013, -0.007, 0.011)
U_WALL = (0.0123, 0.0071, 0.0034)
U_LID = 0.02
U_INLET = 0.03
OMEGAS = (1.0, 1.3, 1.6, 1.9)
STEPS = (2, 3, 4, 5)

BCSpec = namedtuple("BCSpec", "kind id indices params")
Case = namedtuple("Case", "setup background probe pos classes role steps omega seed n")


def case_id(c):
    return f"{c.n:03d}-{c.setup.name}-{c.background}-{c.probe}-{'_'.join(str(v) for v in c.pos)}"


def _faces(shape, remove_edges=False):
    return orc.bounding_box_indices(shape, remove_edges=remove_edges)


def _union(faces, names):
    return np.unique(np.concatenate([np.asarray(faces[s]) for s in names], axis=1), axis=-1).tolist()


def background_specs(background, shape):
    """[(kind, indices, params)] in construction (= id) and list order"""
    box, box_ne = _faces(shape), _faces(shape, remove_edges=True)
    if background == "bare":
        return []
    if background == "plates":  # periodic in x and y; the bottom plate moves
        return [(orc.KIND_HALFWAY_BB, box["top"], {}), (orc.KIND_HALFWAY_BB, box["bottom"], dict(u_wall=U_WALL))]
    if background in ("cavity_hw", "cavity_fw"):  # _util.hip_cavity_3d: [lid, walls]
        kind = orc.KIND_HALFWAY_BB if background == "cavity_hw" else orc.KIND_FULLWAY_BB
        return [(orc.KIND_EQUILIBRIUM, box_ne["top"], dict(rho=1.0, u=(U_LID, 0.0, 0.0))),
                (kind, _union(box, ("bottom", "left", "right", "front", "back")), {})]
    if background == "inout":  # Regularized velocity in, Zou-He pressure out, halfway walls on the other faces (they own the edges)
        return [(orc.KIND_HALFWAY_BB, _union(box, ("bottom", "top", "front", "back")), {}),
                (orc.KIND_REGULARIZED_VELOCITY, box_ne["left"], dict(prescribed=(U_INLET, 0.0, 0.0))),
                (orc.KIND_ZOUHE_PRESSURE, box_ne["right"], dict(prescribed=1.0))]
    raise ValueError(background)


def probe_spec(probe, pos, shape):
    x, y, z = pos
    if probe == "fw":
        return (orc.KIND_FULLWAY_BB, [[x], [y], [z]], {})
    if probe == "eq":
        return (orc.KIND_EQUILIBRIUM, [[x], [y], [z]], dict(rho=1.0, u=U_PROBE))
    if probe == "hw":
        return (orc.KIND_HALFWAY_BB, [[x], [y], [z]], {})
    if probe == "hwm":
        return (orc.KIND_HALFWAY_BB, [[x], [y], [z]], dict(u_wall=U_WALL))
    if probe == "hw2x":  # two adjacent solid cells (DESIGN.md section 3 records an optimisation dropped over this shape)
        x2 = x + 1 if x + 1 < shape[0] else x - 1
        return (orc.KIND_HALFWAY_BB, [[x, x2], [y, y], [z, z]], {})
    if probe == "hw2z":
        z2 = z + 1 if z + 1 < shape[2] else z - 1
        return (orc.KIND_HALFWAY_BB, [[x, x], [y, y], [z, z2]], {})
    raise ValueError(probe)


def bc_specs(setup, background, probe, pos):
    """the stepper's boundary conditions, ids 1, 2, ... in list order; the probe comes last (`probe` None: the background alone)"""
    raw = background_specs(background, setup.shape)
    if probe is not None:
        raw = raw + [probe_spec(probe, pos, setup.shape)]
    return [BCSpec(kind, i + 1, idx, params) for i, (kind, idx, params) in enumerate(raw)]


def oracle_bcs(specs):
    return [orc.BC(s.kind, s.id, s.indices, **s.params) for s in specs]


Masks = namedtuple("Masks", "lat obcs bc_mask missing_mask")


@functools.lru_cache(maxsize=16)
def masks(setup, background, probe, pos):
    lat = orc.Lattice(setup.lattice)
    obcs = oracle_bcs(bc_specs(setup, background, probe, pos))
    if obcs:
        bm, mm = orc.build_masks(setup.shape, lat, obcs)
    else:
        bm, mm = np.zeros((1,) + setup.shape, np.uint8), np.zeros((lat.q,) + setup.shape, bool)
    bm.setflags(write=False)
    mm.setflags(write=False)
    return Masks(lat, obcs, bm, mm)


def case_masks(c):
    return masks(c.setup, c.background, c.probe, c.pos)


def needs_missing(specs):
    """bc_kinds.hpp:12 bc_reads_missing over the stepper's BCs"""
    basic = (orc.KIND_EQUILIBRIUM, orc.KIND_FULLWAY_BB, orc.KIND_DO_NOTHING)
    return any(s.kind not in basic for s in specs)


def restated_plan(c, knobs=KNOBS[0], strips_valid=False, xseg=None):
    """[(Launch, [clean flag per item])] of the next pass of case c under `knobs`"""
    s = c.setup
    specs = bc_specs(s, c.background, c.probe, c.pos)
    ls = pass_launches(s.lattice, s.shape, s.halo, s.overlap, s.xseg if xseg is None else xseg, knobs, needs_missing(specs), s.inout, strips_valid)
    tagged = case_masks(c).bc_mask[0] != 0
    return [(l, clean_flags(tagged, l, s.halo > 0)) for l in ls]


@functools.lru_cache(maxsize=4)
def f_init(c):
    f = orc.perturbed_init(c.setup.shape, orc.Lattice(c.setup.lattice), seed=c.seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=4)  # (the knob sets and variants of a case run back to back: one oracle run per case)
def expected(c, steps=None, probe=True):
    """The oracle's populations after c.steps steps (`probe` False: the same start on the background alone)"""
    m = case_masks(c) if probe else masks(c.setup, c.background, None, None)
    with np.errstate(all="ignore"):  # (the Zou-He expressions are evaluated on every cell and selected afterwards)
        out = orc.run(f_init(c), m.bc_mask, m.missing_mask, m.obcs, c.omega, m.lat, c.steps if steps is None else steps)
    out.setflags(write=False)
    return out


# ---- positions -----------------------------------------------------------------------------------------------------------------------
SEAM_OFFSETS = (-2, -1, 0, 1)
SWEEP_X_OFFSETS = (-2, -1, 0, 2)  # x_lo - 1 and x_lo: the rim planes of the two items at the boundary; - 2 and + 2: one further out
YZ_TYPES = ("seam-2", "seam-1", "seam+0", "seam+1", "wrap_lo", "wrap_hi", "interior")
X_TYPES = ("lo-2", "lo-1", "lo+0", "lo+1", "lo+2", "wrap_lo", "wrap_hi")
WALL_Z_TYPES = ("z1", "z2", "znz-3", "znz-2")


def default_launches(setup):
    return pass_launches(setup.lattice, setup.shape, setup.halo, setup.overlap, setup.xseg, KNOBS[0], True, setup.inout)


def seams(setup, axis):
    """tile boundaries of the shifted tiling along y (axis 1) or z (axis 2)"""
    tile, n = step2_tile(setup.lattice), setup.shape[axis]
    t, o = tile[axis - 1], tile_shift(tile)[axis - 1]
    return sorted({(k * t + o) % n for k in range(n // t)})


def segment_starts(setup):
    """x_lo of every item of every launch of the default plan"""
    return sorted({it[1] for l in default_launches(setup) for it in l.items})


def interior_coord(setup, axis):
    """a coordinate in the middle of the first tile of the axis (of the widest x segment for axis 0)"""
    if axis == 0:
        lo, hi = max(((it[1], it[2]) for l in default_launches(setup) for it in l.items), key=lambda r: (r[1] - r[0], -r[0]))
        return (lo + (hi - lo) // 2) % setup.shape[0]
    tile = step2_tile(setup.lattice)
    return (seams(setup, axis)[0] + tile[axis - 1] // 2) % setup.shape[axis]


def class_coord(setup, axis, ctype, instance):
    """the coordinate of a class type on an axis; `instance` picks the seam / segment"""
    n = setup.shape[axis]
    if ctype == "wrap_lo":
        return 0
    if ctype == "wrap_hi":
        return n - 1
    if ctype == "interior":
        return interior_coord(setup, axis)
    if ctype in WALL_Z_TYPES:
        return {"z1": 1, "z2": 2, "znz-3": n - 3, "znz-2": n - 2}[ctype]
    base, off = ctype[:-2], int(ctype[-2:])
    where = segment_starts(setup) if base == "lo" else seams(setup, axis)
    return (where[instance % len(where)] + off) % n


def _keeps_clean_and_dirty_items(setup, background, probe, pos):
    return keeps_clean_and_dirty_items(Case(setup, background, probe, pos, None, None, 0, 0.0, 0, 0))


def keeps_clean_and_dirty_items(c):
    """a case whose pass has a launch of three or more segments has a clean and a dirty item among the items that read flags"""
    plan = [(l, flags) for l, flags in restated_plan(c) if l.has_flags]
    if not any(l.segments >= 3 for l, _ in plan):
        return True
    flags = [f for _, fs in plan for f in fs]
    return 0 in flags and 1 in flags


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(setup, background, probe, pos, classes, role):
        n = len(out)
        out.append(Case(setup, background, probe, tuple(int(v) for v in pos), classes, role, STEPS[n % 4], OMEGAS[(n // 4) % 4], 2000 + n, n))

    rot = 0  # (probe, round) combinations of the rotation block dealt so far
    turn = 0  # classes handed to the wall backgrounds so far
    z_turn = {}  # ... z classes, per background: the positions next to the wall lanes come first
    plain = [s for s in SETUPS if not s.inout]
    for si, setup in enumerate(SETUPS):
        inner = [interior_coord(setup, a) for a in range(3)]
        if not setup.inout:
            # sweep: one axis at a time across every boundary of the plan
            k = 0
            for axis in range(3):
                if axis > 0 and setup.shape[axis] == step2_tile(setup.lattice)[axis - 1]:
                    continue  # a single tile along this axis: its rim holds periodic images of its own cells only
                where = segment_starts(setup) if axis == 0 else seams(setup, axis)
                for i, b in enumerate(where):
                    for off in SWEEP_X_OFFSETS if axis == 0 else SEAM_OFFSETS:
                        pos = list(inner)
                        pos[axis] = (b + off) % setup.shape[axis]
                        name = f"{'lo' if axis == 0 else 'seam'}{off:+d}"
                        classes = tuple(name if a == axis else "interior" for a in range(3))
                        add(setup, "bare", PROBES[k % 2], pos, classes, ("sweep", axis, i, off))
                        k += 1
            # rotation: every probe kind x every class type of every axis over the set-ups (42 combinations, 6 per set-up)
            for _ in range(len(PROBES) * len(X_TYPES) // len(plain)):
                p, r = rot % len(PROBES), rot // len(PROBES)
                classes = (X_TYPES[r % 7], YZ_TYPES[(r + 2) % 7], YZ_TYPES[(r + 4) % 7])
                pos = [class_coord(setup, a, classes[a], rot + a) for a in range(3)]
                add(setup, "bare", PROBES[p], pos, classes, ("rotation", p, r))
                rot += 1
        for bi, background in enumerate(b for b in setup.backgrounds if b != "bare"):
            z_types = WALL_Z_TYPES + YZ_TYPES
            x_types = X_TYPES[:5] if setup.inout else X_TYPES  # (the end planes belong to the inlet and the outlet)
            for j in range(6 if setup.inout else 3):
                while True:  # the next turn whose probe leaves a clean and a dirty item in every launch of three or more segments
                    zt = z_turn.get(background, 0)
                    classes = (x_types[turn % len(x_types)], YZ_TYPES[(turn // 2 + 3) % 7], z_types[zt % len(z_types)])
                    pos = tuple(class_coord(setup, a, classes[a], turn + a) for a in range(3))
                    probe = PROBES[(turn + j) % len(PROBES)]
                    turn += 1
                    z_turn[background] = zt + 1
                    if _keeps_clean_and_dirty_items(setup, background, probe, pos):
                        break
                add(setup, background, probe, pos, classes, ("walls", j))
            if background in ("plates", "cavity_hw", "inout"):
                # a halfway solid touching the wall z = 0: its diagonal neighbours (x +- 1, y +- 1, z = 1) gain an x-y bit, one lane per row
                add(setup, background, "hw", (inner[0], inner[1], 1), ("interior", "interior", "z1"), ("arm",))
            if (si + bi) % 3 == 0:
                add(setup, background, PROBES[(si + bi) % 2], (inner[0], 1, 1), ("interior", "edge", "edge"), ("yz_edge",))
    return tuple(out)


def knob_sets(c):
    """the knob sets a case runs under: the defaults, and each alternative for a rotating third of the table"""
    return (KNOBS[0],) + tuple(k for a, k in enumerate(KNOBS[1:]) if (c.n + a) % 3 == 0)


def runs_reference_protocol(c):
    """a rotating tenth of the table also runs as stepper(f_0, f_1, ...) calls with the caller's swap"""
    return c.n % 10 == 3
