"""Conditions on the case generator of the single-step kernel's matrix (tests/_step_matrix.py), checked with the oracle alone: the
GPU test that runs these cases (tests/test_gpu_step_matrix.py) cannot pass vacuously — every template combination the launcher can
instantiate is asked for, every case computes something, storage rounding and the moving wall really enter the result, and the
boundary cells sit where the packed bc_mask loads of the VEC > 1 kernels can go wrong."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _step_matrix as sm

CASES = sm.cases()
RUN = [c for c in CASES if not c.refused]

# ---- what step_launch.hpp can instantiate, written out: (lattice, collision, policy, VEC, HASBC) ---------------------------------
# launch_step: five policies; launch_policy: VEC 4 for 4-byte compute types only; launch_vec: HASBC 0, 1, 2
_VECS = {"FP32FP32": (1, 2, 4), "FP32FP16": (1, 2, 4), "FP64FP64": (1, 2), "FP64FP32": (1, 2), "FP64FP16": (1, 2)}
_PLAIN = [("D2Q9", "BGK"), ("D2Q9", "KBC"), ("D3Q19", "BGK"), ("D3Q27", "BGK"), ("D3Q27", "KBC")]
# launch_step_ext: three policies (of the variants in step_<lattice>_ext.hip the matrix takes Smagorinsky and the forced BGK)
_EXT = [(lattice, coll) for lattice in ("D2Q9", "D3Q19", "D3Q27") for coll in ("SmagorinskyLESBGK", "ForcedBGK")]
_EXT_POLICIES = ("FP32FP32", "FP64FP64", "FP64FP32")
EXPECTED = {(la, co, po, v, h) for la, co in _PLAIN for po in _VECS for v in _VECS[po] for h in (0, 1, 2)}
EXPECTED |= {(la, co, po, v, h) for la, co in _EXT for po in _EXT_POLICIES for v in _VECS[po] for h in (0, 1, 2)}
REFUSED = {(la, co, po) for la, co in _EXT for po in ("FP32FP16", "FP64FP16")}

FP16_MIN_NORMAL, FP16_MAX = 2.0**-14, 65504.0


def effective_vec(c):
    return sm.pick_vec(c.policy, c.shape[-1], c.vec)


def test_expected_table_size():
    assert len(EXPECTED) == 5 * 12 * 3 + 6 * 7 * 3 and len(REFUSED) == 12


def test_every_instantiable_combination_is_a_case():
    got = {(c.lattice, c.collision, c.policy, effective_vec(c), sm.HASBC[c.bc_class]) for c in RUN}
    assert got == EXPECTED, (sorted(EXPECTED - got), sorted(got - EXPECTED))
    assert {(c.lattice, c.collision, c.policy) for c in CASES if c.refused} == REFUSED
    assert all(c.collision in ("SmagorinskyLESBGK", "ForcedBGK") and c.policy.endswith("FP16") for c in CASES if c.refused)
    # the table-lookup class runs every lattice, policy and effective VEC
    many = {(c.lattice, c.policy, effective_vec(c)) for c in RUN if c.bc_class == "many"}
    assert many == {(la, po, v) for la in ("D2Q9", "D3Q19", "D3Q27") for po in _VECS for v in _VECS[po]}


def test_case_ids_are_unique_and_requested_vecs_are_the_built_ones():
    ids = [sm.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert c.vec in _VECS[c.policy]


def test_shapes_reach_every_index_path():
    groups = {}
    for c in RUN:
        groups.setdefault((c.lattice, c.collision, c.policy, c.vec, c.bc_class), []).append(c)
    for (lattice, coll, policy, vec, bc_class), cs in groups.items():
        nzs = {c.shape[-1] for c in cs}
        if bc_class == "none":
            # both row ends in one thread, one thread per row end, a middle thread
            assert {vec, 2 * vec, 3 * vec} <= nzs, (lattice, coll, policy, vec)
            others = {c.shape[:-1] for c in cs}
            assert len(others) == 4  # the four (nx, ny) of the generator, each once
        if bc_class in ("none", "basic", "extended") and vec > 1:
            assert any(nz % vec != 0 for nz in nzs), "no shape on which pick_vec falls back to one cell per thread"
            assert any(nz % vec == 0 for nz in nzs)
        if bc_class != "none":
            for c in cs:
                assert all(n >= 6 for n in c.shape), "no room for the interior solid two cells from every face"
    # nz = 6 with vec 4 and nz = 7 with vec 2 are the fallbacks
    assert any(c.vec == 4 and c.shape[-1] == 6 for c in RUN) and any(c.vec == 2 and c.shape[-1] == 7 for c in RUN)
    # periodic boxes: the x wrap onto both neighbours at once (nx = 1, 2), ny == 1, for every requested vec and every kernel row end
    for vec in (1, 2, 4):
        for role in (1, 2, 3):
            sel = [c for c in RUN if c.bc_class == "none" and c.vec == vec and c.shape[-1] == role * vec and c.lattice != "D2Q9"]
            assert {c.shape[:2] for c in sel} == {(1, 3), (2, 5), (3, 1), (5, 6)}, (vec, role)
            sel2 = [c for c in RUN if c.bc_class == "none" and c.vec == vec and c.shape[-1] == role * vec and c.lattice == "D2Q9"]
            assert {c.shape[0] for c in sel2} == {1, 2, 3, 5}, (vec, role)
    steps = {c.steps for c in RUN}
    assert steps == {3, 4, 5}
    for key in {(c.lattice, c.collision, c.policy, sm.HASBC[c.bc_class]) for c in RUN}:
        assert {c.steps % 2 for c in RUN if (c.lattice, c.collision, c.policy, sm.HASBC[c.bc_class]) == key} == {0, 1}, key


def test_every_kind_of_a_class_occurs():
    kinds = {cl: set() for cl in sm.BC_CLASSES}
    for c in RUN:
        kinds[c.bc_class] |= {s.kind for s in sm.bc_specs(c)[0]}
    basic = {orc.KIND_EQUILIBRIUM, orc.KIND_FULLWAY_BB, orc.KIND_DO_NOTHING, orc.KIND_HALFWAY_BB}
    assert kinds["none"] == set() and kinds["basic"] == basic and kinds["many"] == basic
    assert kinds["extended"] == {orc.KIND_REGULARIZED_VELOCITY, orc.KIND_ZOUHE_VELOCITY, orc.KIND_ZOUHE_PRESSURE, orc.KIND_EXTRAPOLATION_OUTFLOW,
                                 orc.KIND_HALFWAY_BB}
    # ... and both inlet / outlet pairs meet every lattice, policy and requested vec
    for lattice in ("D2Q9", "D3Q19", "D3Q27"):
        for policy in sm.POLICIES:
            for vec in _VECS[policy]:
                sel = [c for c in RUN if c.bc_class == "extended" and (c.lattice, c.policy, c.vec) == (lattice, policy, vec)]
                assert {sm.extended_variant(c) for c in sel} == {0, 1}, (lattice, policy, vec)


@pytest.mark.parametrize("c", RUN, ids=sm.case_id)
def test_case_computes_something(c):
    exp = sm.expected(c)
    assert exp.dtype == orc.store_dtype(c.policy) and exp.shape == (orc.Lattice(c.lattice).q,) + c.shape
    e64 = exp.astype(np.float64)
    assert np.isfinite(e64).all() and (e64 > 0).all()
    if c.policy.endswith("FP16"):
        assert e64.min() >= FP16_MIN_NORMAL and e64.max() <= FP16_MAX
        # the same case with 4-byte storage: rounding to the store type really happens
        wide = sm.expected(c, policy=c.policy[:4] + "FP32")
        assert wide.dtype == np.float32 and not np.array_equal(wide.astype(np.float64), e64)
    if c.bc_class in ("basic", "many"):
        at_rest = sm.expected(c, moving=False)
        assert not np.array_equal(at_rest, exp), "the moving wall does not enter the result"
    if c.policy in ("FP32FP16", "FP64FP32", "FP64FP16") and c.bc_class in ("basic", "many"):
        # the wall term 6 w (c . u_wall) is summed in the STORE type (bc_halfway_bounce_back.py:97-102): for the mixed policies the
        # sum in the compute type is another number, in a direction that the wall really replaces
        assert _wall_term_depends_on_the_store_type(c)


def _wall_term_depends_on_the_store_type(c):
    s = sm.setup(c)
    lat = s.lat
    T, S = orc.compute_dtype(c.policy), orc.store_dtype(c.policy)
    mov = next(b for b in s.obcs if b.u_wall is not None)
    missing_here = (s.missing_mask & (s.bc_mask == mov.id)).reshape(lat.q, -1).any(axis=1)
    uw = np.asarray(mov.u_wall, dtype=np.float64).astype(S)
    for l in np.nonzero(missing_here)[0]:
        in_store, in_compute = S(0), T(0)
        for d in range(lat.d):
            in_store = S(in_store + S(int(lat.c[d, l])) * uw[d])
            in_compute = T(in_compute + T(int(lat.c[d, l])) * T(uw[d]))
        if T(in_store) != in_compute:
            return True
    return False


@pytest.mark.parametrize("c", [c for c in RUN if c.bc_class != "none"], ids=sm.case_id)
def test_boundary_cells_of_a_case(c):
    s = sm.setup(c)
    specs, order = sm.bc_specs(c)
    assert [b.id for b in s.obcs] == [specs[i].id for i in order] and [sp.id for sp in specs] == list(range(1, len(specs) + 1))
    assert [b.id for b in s.obcs] != sorted(b.id for b in s.obcs), "list order equals id order"
    ids = s.bc_mask[0]
    for b in s.obcs:
        assert (ids == b.id).any(), f"BC {b.id} ({b.kind}) tags no cell"
    if c.bc_class == "many":
        assert len(s.obcs) > sm.MAX_FAST_BCS
    else:
        assert len(s.obcs) <= sm.MAX_FAST_BCS
    # a halfway / Zou-He / outflow cell that misses a direction with c_z != 0 (the z-shifted loads feed the populations they replace)
    cz = s.lat.c[-1]
    uses_missing = [b.id for b in s.obcs if b.kind not in (orc.KIND_EQUILIBRIUM, orc.KIND_FULLWAY_BB, orc.KIND_DO_NOTHING)]
    assert (s.missing_mask[cz != 0] & np.isin(ids, uses_missing)[None]).any()
    # fluid between opposite faces: away from the faces' planes some cell carries no id
    assert (ids[(slice(1, -1),) * s.lat.d] == 0).any()
    vec = effective_vec(c)
    if vec > 1:
        z = np.nonzero(ids)[-1]
        nz = c.shape[-1]
        assert (z < vec).any(), "no boundary cell in the first vector of a row"
        assert (z >= nz - vec).any(), "no boundary cell in the last vector of a row"
        assert (z % 2 == 1).any(), "no boundary cell at an odd z"
        # every byte lane of the packed bc_mask word carries an id somewhere, and some word mixes ids with fluid
        assert {int(v) for v in z % vec} == set(range(vec))
        words = ids.reshape(-1, vec)
        assert ((words != 0).any(axis=1) & (words == 0).any(axis=1)).any()


def test_knob_geometries_reach_the_swizzle():
    """The arithmetic of the comment at sm.KNOB_GEOMETRIES: the swizzle is live in two geometries, one per block size, both with a partial last block
    row, and switches itself off in the others."""
    assert sm.launch_grid((3, 30, 128), 1, 64, 256) == (2, 8, 3) and 8 * 4 > 30
    assert sm.launch_grid((3, 30, 128), 1, 64, 128) == (2, 15, 3)
    assert sm.launch_grid((3, 15, 128), 1, 64, 128) == (2, 8, 3) and 8 * 2 > 15
    assert sm.launch_grid((3, 20, 128), 1, 64, 256) == (2, 5, 3)
    assert sm.launch_grid((3, 30, 128), 4, 16, 256) == (2, 2, 3) and sm.launch_grid((3, 30, 128), 4, 16, 128) == (2, 4, 3)
    on = [(g, t) for g in sm.KNOB_GEOMETRIES for t in (128, 256) if sm.swizzle_active(*g, t)]
    assert on == [(((3, 30, 128), 1, 64), 256), (((3, 15, 128), 1, 64), 128)]
