"""The case matrix of the single-step kernel k_step<L, T, S, VEC, COLL, HASBC, FLAGS> (csrc/step_kernel.hpp) and the oracle side
of every case.  No GPU and no xlb_amd here: tests/test_step_matrix_cases.py checks the generator with the oracle alone, and
tests/test_gpu_step_matrix.py builds the matching xlb_amd objects from the same records.

Axes (step_launch.hpp): lattice x collision as built, the five precision policies, the requested cells per thread, and the
boundary-condition variant of the kernel (HASBC 0 / 1 / 2).  The shapes are the smallest at which an index path of the kernel can
still go wrong; "nz" is the last axis (the second of the two for D2Q9), the one a thread's VEC cells run along:

  periodic   nz in {VEC, 2 VEC, 3 VEC} (both row ends in one thread; one thread per row end; a middle thread) and one nz that the
             requested vec does not divide (pick_vec falls back to 1), each paired with one of (1, 3), (2, 5), (3, 1), (5, 6) for
             the other axes: nx in {1, 2} wraps x onto both neighbours at once, ny == 1 wraps y onto itself.  The pairing rotates
             from one combination to the next, so every (nz, other axes) pair occurs on every lattice.
  BC classes (7, 6, nz): one fluid cell or more between opposite faces, the interior solid two cells from every face, which
             takes nz >= 6 — so VEC < nz here, and the row ends are two threads.

Every (lattice, collision, policy, vec) gets every nz of its list in every class: the full product, about 1200 cases of a few
milliseconds each."""

import functools
from collections import namedtuple

import numpy as np

from oracle import xlb_numpy as orc

POLICIES = ("FP32FP32", "FP32FP16", "FP64FP64", "FP64FP32", "FP64FP16")
# the collisions as built: step_<lattice>_<collision>.hip, and the extended ones of step_<lattice>_ext.hip
PLAIN = (("D2Q9", "BGK"), ("D2Q9", "KBC"), ("D3Q19", "BGK"), ("D3Q27", "BGK"), ("D3Q27", "KBC"))
EXTENDED = tuple((lattice, coll) for lattice in ("D2Q9", "D3Q19", "D3Q27") for coll in ("SmagorinskyLESBGK", "ForcedBGK"))
EXT_POLICIES = ("FP32FP32", "FP64FP64", "FP64FP32")
EXT_REFUSAL = "built for FP32FP32, FP64FP64 and FP64FP32 only"  # launch_step_ext's message
BC_CLASSES = ("none", "basic", "extended", "many")
HASBC = {"none": 0, "basic": 1, "many": 1, "extended": 2}
MAX_FAST_BCS = 8  # cell.hpp: more boundary conditions than this take the bc_kind[] table

U_WALL = (0.0123, 0.0071, 0.0034)  # no component is an fp16 (or fp32) number, nor is any sum of two
U_LID = (0.02, 0.0, 0.01)
U_INLET = 0.03
FORCE = (1e-5, 3e-6, -2e-6)

Case = namedtuple("Case", "lattice collision policy vec bc_class shape steps omega seed refused")
# a boundary condition of a case: ids are handed out in construction order (`id`), the list order differs
BCSpec = namedtuple("BCSpec", "kind id indices params")


def requested_vecs(policy):
    return (1, 2, 4) if policy.startswith("FP32") else (1, 2)


def pick_vec(policy, nz, requested):
    """step_launch.hpp: pick_vec"""
    vmax = 4 if policy.startswith("FP32") else 2
    v = requested if requested > 0 else 1
    v = min(v, vmax)
    if v == 3:
        v = 2
    if nz % v != 0:
        v = 1
    return v


def case_id(c):
    return f"{c.lattice}-{c.collision}-{c.policy}-vec{c.vec}-{c.bc_class}-{'x'.join(str(s) for s in c.shape)}" + ("-refused" if c.refused else "")


def collision_args(c):
    """(collision_type, force_vector) as the stepper and orc.run take them"""
    d = 2 if c.lattice == "D2Q9" else 3
    if c.collision == "ForcedBGK":
        return "BGK", FORCE[:d]
    return c.collision, None


def _nz_list(vec, bc_class):
    if bc_class == "none":
        return {1: (1, 2, 3, 5), 2: (2, 4, 6, 7), 4: (4, 8, 12, 6)}[vec]
    return {1: (6, 7), 2: (6, 8, 7), 4: (8, 12, 6)}[vec]


_OTHER_AXES = ((1, 3), (2, 5), (3, 1), (5, 6))
_OMEGAS = (1.0, 1.3, 1.7, 1.9)


def _shape(lattice, bc_class, nz, k):
    if bc_class == "none":
        other = _OTHER_AXES[k % 4]
        return (other[0], nz) if lattice == "D2Q9" else other + (nz,)
    return (7, nz) if lattice == "D2Q9" else (7, 6, nz)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    turn = {}  # combinations so far per (lattice, vec): rotates the pairing of nz with the other axes
    for bc_class in BC_CLASSES:
        for lattice, coll in PLAIN + EXTENDED:
            ext = (lattice, coll) in EXTENDED
            for policy in POLICIES:
                refused = ext and policy not in EXT_POLICIES
                for vec in requested_vecs(policy):
                    if refused and (vec != 1 or bc_class != "none"):
                        continue  # one refusal per (lattice, collision, policy): launch_step_ext refuses before vec or HASBC matter
                    k = turn.get((lattice, vec), 0)
                    for j, nz in enumerate(_nz_list(vec, bc_class)[: 1 if refused else None]):
                        n = len(out)
                        out.append(Case(lattice, coll, policy, vec, bc_class, _shape(lattice, bc_class, nz, k + j), 3 + n % 3,
                                        _OMEGAS[(n // 3) % 4], 1000 + n, refused))
                    turn[(lattice, vec)] = k + 1
    return tuple(out)


# ---- boundary conditions ----------------------------------------------------------------------------------------------------------
def _faces(shape, remove_edges=True):
    return orc.bounding_box_indices(shape, remove_edges=remove_edges)


def _select(indices, keep):
    a = np.asarray(indices)
    return a[:, keep(a)].tolist()


def _interior_solid(shape):
    """2 x 2 (x 2) cells, two cells or more from every face"""
    lo = [3, 2] if len(shape) == 2 else [3, 2, 2]
    g = np.meshgrid(*[np.arange(a, a + 2) for a in lo], indexing="ij")
    return [x.ravel().tolist() for x in g]


def _basic(shape, strips, moving=True):
    """(specs in construction order, list order).  3-D: lid on the top face (z = nz - 1), moving halfway wall on the bottom (z = 0),
    fullway on the left (x = 0), do-nothing on the right, no-slip halfway on the front (y = 0), the back open.  2-D has four faces:
    top / bottom / right as above (the row ends are y = 0 and y = ny - 1), the left face shared by the fullway (lower half) and
    the no-slip halfway wall (upper half).  `strips`: the do-nothing face cut along the second axis into one BC per strip."""
    d = len(shape)
    f = _faces(shape)
    if d == 3:
        fullway, noslip = f["left"], f["front"]
    else:
        half = shape[1] // 2
        fullway = _select(f["left"], lambda a: a[1] < half)
        noslip = _select(f["left"], lambda a: a[1] >= half)
    u_wall = U_WALL[:d] if moving else (0.0,) * d
    raw = [
        (orc.KIND_EQUILIBRIUM, f["top"], dict(rho=1.0, u=U_LID if d == 3 else U_LID[:2])),
        (orc.KIND_HALFWAY_BB, f["bottom"], dict(u_wall=u_wall)),
        (orc.KIND_FULLWAY_BB, fullway, {}),
        (orc.KIND_HALFWAY_BB, _interior_solid(shape), {}),
        (orc.KIND_HALFWAY_BB, noslip, {}),
    ]
    if strips:
        right = np.asarray(f["right"])
        for v in np.unique(right[1]):
            raw.append((orc.KIND_DO_NOTHING, right[:, right[1] == v].tolist(), {}))
    else:
        raw.append((orc.KIND_DO_NOTHING, f["right"], {}))
    specs = [BCSpec(kind, i + 1, idx, params) for i, (kind, idx, params) in enumerate(raw)]
    n = len(specs)
    order = [3, 2, 0] + list(range(n - 1, 4, -1)) + [1, 4]  # solid, fullway, lid, do-nothing (strips backwards), moving, no-slip
    assert sorted(order) == list(range(n)) and order != sorted(order)
    return specs, order


def _extended(shape, variant):
    """Velocity inlet on the left face, outlet on the right, halfway walls on every other face (edges included: they own the corners).
    variant 0: Regularized velocity + Zou-He pressure; 1: Zou-He velocity + extrapolation outflow"""
    d = len(shape)
    f, full = _faces(shape), _faces(shape, remove_edges=False)
    sides = ["bottom", "top"] + (["front", "back"] if d == 3 else [])
    walls = np.unique(np.concatenate([np.asarray(full[s]) for s in sides], axis=1), axis=-1).tolist()
    u_in = (U_INLET,) + (0.0,) * (d - 1)
    if variant == 0:
        inlet = (orc.KIND_REGULARIZED_VELOCITY, f["left"], dict(prescribed=u_in))
        outlet = (orc.KIND_ZOUHE_PRESSURE, f["right"], dict(prescribed=1.0))
    else:
        inlet = (orc.KIND_ZOUHE_VELOCITY, f["left"], dict(prescribed=u_in))
        outlet = (orc.KIND_EXTRAPOLATION_OUTFLOW, f["right"], {})
    raw = [outlet, (orc.KIND_HALFWAY_BB, walls, {}), inlet]
    specs = [BCSpec(kind, i + 1, idx, params) for i, (kind, idx, params) in enumerate(raw)]
    return specs, [1, 2, 0]  # walls, inlet, outlet (the order of examples/cfd/flow_past_sphere_3d.py:108-112)


def extended_variant(c):
    """both inlet / outlet pairs for every (lattice, collision, policy, vec): the nz of its list take them in turn"""
    return (POLICIES.index(c.policy) + c.vec + _nz_list(c.vec, "extended").index(c.shape[-1])) % 2


def bc_specs(c, moving=True):
    """(specs in construction order — ids 1, 2, ... —, the positions of the stepper's list in it)"""
    if c.bc_class == "none":
        return [], []
    if c.bc_class == "extended":
        return _extended(c.shape, extended_variant(c))
    return _basic(c.shape, strips=c.bc_class == "many", moving=moving)


def oracle_bcs(specs, order):
    return [orc.BC(specs[i].kind, specs[i].id, specs[i].indices, **specs[i].params) for i in order]


Setup = namedtuple("Setup", "lat obcs bc_mask missing_mask f_init")


@functools.lru_cache(maxsize=None)
def setup(c, moving=True):
    lat = orc.Lattice(c.lattice)
    specs, order = bc_specs(c, moving)
    obcs = oracle_bcs(specs, order)
    if obcs:
        bm, mm = orc.build_masks(c.shape, lat, obcs)
    else:
        bm, mm = np.zeros((1,) + c.shape, np.uint8), np.zeros((lat.q,) + c.shape, bool)
    f_init = orc.perturbed_init(c.shape, lat, c.policy, seed=c.seed, amp_rho=0.02, amp_u=0.03)
    for a in (bm, mm, f_init):
        a.setflags(write=False)
    return Setup(lat, obcs, bm, mm, f_init)


def expected(c, policy=None, moving=True):
    """The oracle's populations after c.steps steps; `policy` / `moving` vary the case for the generator's own checks"""
    s = setup(c, moving)
    coll, force = collision_args(c)
    with np.errstate(all="ignore"):  # (the Zou-He expressions are evaluated on every cell and selected afterwards)
        return orc.run(s.f_init, s.bc_mask, s.missing_mask, s.obcs, c.omega, s.lat, c.steps, policy or c.policy, coll, force)


# ---- launch knobs ------------------------------------------------------------------------------------------------------------------
# launch_typed (step_launch.hpp) with nzq = nz / VEC cells along z per row, `threads` = block_threads:
#   tz = min(nzq, threads, block_tz), ty = min(threads / tz, ny), grid = (ceil(nzq / tz), ceil(ny / ty), nx),
#   the swizzle is on when grid.x > 1 and grid.y % 8 == 0.
#   (3, 30, 128) vec 1 block_tz 64, 256 threads: tz = 64, ty = 4, grid = (2, 8, 3); the last block row holds y = 28, 29 of 28..31: ON
#   (3, 30, 128) vec 1 block_tz 64, 128 threads: tz = 64, ty = 2, grid = (2, 15, 3): off
#   (3, 15, 128) vec 1 block_tz 64, 128 threads: tz = 64, ty = 2, grid = (2, 8, 3); the last block row holds y = 14 of 14..15: ON
#   (3, 20, 128) vec 1 block_tz 64, 256 threads: tz = 64, ty = 4, grid = (2, 5, 3): the swizzle must switch itself off
#   (3, 30, 128) vec 4 block_tz 16: nzq = 32, tz = 16, ty = 16 (256 threads) / 8 (128), grid = (2, 2, 3) / (2, 4, 3): off
KNOB_GEOMETRIES = [((3, 30, 128), 1, 64), ((3, 15, 128), 1, 64), ((3, 20, 128), 1, 64), ((3, 30, 128), 4, 16)]


def launch_grid(shape, vec, block_tz, threads):
    """launch_typed's block and grid, restated"""
    ceil_div = lambda a, b: -(-a // b)  # noqa: E731
    nzq, ny = shape[2] // vec, shape[1]
    tz = nzq
    if tz > threads:
        tz = min(ceil_div(ceil_div(nzq, ceil_div(nzq, threads)), 64) * 64, threads)
    if 0 < block_tz < tz:
        tz = block_tz
    ty = max(1, min(threads // tz, ny))
    return (ceil_div(nzq, tz), ceil_div(ny, ty), shape[0])


def swizzle_active(shape, vec, block_tz, threads):
    gx, gy, _ = launch_grid(shape, vec, block_tz, threads)
    return gx > 1 and gy % 8 == 0
