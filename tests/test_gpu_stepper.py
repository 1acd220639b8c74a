"""Parity of the fused HIP stepper (through the C ABI) with the oracle and with the committed
golden fixtures.  fp32/fp64 results are expected to be BIT-IDENTICAL to the oracle (same
operation order, no FMA contraction); the asserted bar is the north-star tolerance
(|delta rho|, |delta u| <= 1e-6 in fp32) plus bit-exact integer masks."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import FullwayBounceBackBC, HalfwayBounceBackBC, EquilibriumBC, DoNothingBC
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

from _util import golden, hip_cavity_2d, hip_cavity_3d, hip_macroscopic, init_hip, max_ulp_diff, remap_ids

pytestmark = pytest.mark.gpu

TOL = 1e-6  # BASELINE.json north_star: rho/u within 1e-6 in fp32


def run_reference_loop(stepper, f_0, f_1, bc_mask, missing_mask, omega, n, t0=0):
    """The caller loop of the reference drivers (lid_driven_cavity_2d.py:64-67)."""
    for i in range(n):
        f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, omega, t0 + i)
        f_0, f_1 = f_1, f_0
    return f_0, f_1


@pytest.mark.parametrize("n", [16, 128])
def test_config1_d2q9_cavity_vs_golden(n):
    """BASELINE config 1: D2Q9 BGK lid-driven cavity 128x128 fp32 (and its 16x16 twin)."""
    g = golden(f"d2q9_cavity_{n}")
    grid, bcs, lat, obcs = hip_cavity_2d(n)
    vs, pp = bcs[0].velocity_set, bcs[0].precision_policy
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs, collision_type="BGK")
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    # masks: bit-exact (golden ids are lid=1, walls=2; this process's ids may differ)
    ids = {bcs[1].id: 1, bcs[0].id: 2}
    assert np.array_equal(remap_ids(bc_mask.numpy(), ids), g["bc_mask"])
    assert np.array_equal(missing_mask.numpy(), g["missing_mask"])
    omega = float(g["omega"])
    done = 0
    for s in g["steps"]:
        s = int(s)
        if s - done <= 10:
            f_0, f_1 = run_reference_loop(stepper, f_0, f_1, bc_mask, missing_mask, omega, s - done, done)
        else:
            f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, s - done, first_timestep=done)
        done = s
        rho, u = hip_macroscopic(f_0, grid, vs, pp)
        # boundary ring stripped as the reference post-processing does (lid_driven_cavity_2d.py:89-90) ...
        assert np.abs(rho - g[f"rho_{s}"])[:, 1:-1, 1:-1].max() <= TOL
        assert np.abs(u - g[f"u_{s}"])[:, 1:-1, 1:-1].max() <= TOL
        # ... and the whole field too, which is stronger
        assert np.abs(rho - g[f"rho_{s}"]).max() <= TOL and np.abs(u - g[f"u_{s}"]).max() <= TOL
        assert max_ulp_diff(rho, g[f"rho_{s}"]) == 0 and max_ulp_diff(u, g[f"u_{s}"]) == 0
        if n <= 16:
            assert np.array_equal(f_0.numpy(), g[f"f_{s}"])


@pytest.mark.parametrize("omega", [1.0, 1.7])
def test_config2_twin_d3q19_periodic_vs_golden(omega):
    """BASELINE config 2 twin: D3Q19 BGK periodic, perturbed init (16^3 golden)."""
    g = golden("d3q19_periodic_16")
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    shape = (16, 16, 16)
    grid = grid_factory(shape)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type="BGK")
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_0.assign(orc.perturbed_init(shape, lat, seed=int(g["seed"])))
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, int(g["steps"]))
    out = f_0.numpy()
    assert np.abs(out - g[f"f_omega{omega}"]).max() <= TOL
    assert np.array_equal(out, g[f"f_omega{omega}"])


@pytest.mark.parametrize("walls_cls,tag", [(FullwayBounceBackBC, "fullway"), (HalfwayBounceBackBC, "halfway")])
def test_config3_twin_d3q19_cavity_vs_golden(walls_cls, tag):
    """BASELINE config 3 twin: D3Q19 BGK cavity, both wall treatments (16^3 golden)."""
    g = golden("d3q19_cavity_16")
    grid, bcs, lat, obcs = hip_cavity_3d((16, 16, 16), walls_cls)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs, collision_type="BGK")
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    assert np.array_equal(remap_ids(bc_mask.numpy(), {bcs[0].id: 1, bcs[1].id: 2}), g["bc_mask"])
    assert np.array_equal(np.packbits(missing_mask.numpy(), axis=0), g["missing_mask"])
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, int(g["steps"]))
    out = f_0.numpy()
    assert np.abs(out - g[f"f_{tag}"]).max() <= TOL
    assert np.array_equal(out, g[f"f_{tag}"])


@pytest.mark.parametrize("policy", ["FP64FP32", "FP32FP32", "FP64FP64"])
def test_config5_twin_d3q27_kbc_vs_golden(policy, exact_math):
    """BASELINE config 5 twin: D3Q27 KBC, mixed precision (12^3 golden); bit-exact builds (the default fast fp64
    collision is covered by tests/test_gpu_fastmath.py)."""
    g = golden("d3q27_kbc_12")
    vs, pp = init_hip("D3Q27", policy)
    lat = orc.Lattice("D3Q27")
    shape = (12, 12, 12)
    grid = grid_factory(shape)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type="KBC")
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_0.assign(orc.perturbed_init(shape, lat, policy, seed=0))
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, float(g["omega"]), int(g["steps"]))
    out = f_0.numpy()
    tol = TOL if policy != "FP64FP64" else 1e-12
    assert np.abs(out.astype(np.float64) - g[f"f_{policy}"]).max() <= tol
    assert np.array_equal(out, g[f"f_{policy}"])


def test_d2q9_kbc_cavity_vs_golden():
    g = golden("d2q9_kbc_cavity_16")
    grid, bcs, lat, obcs = hip_cavity_2d(16)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs, collision_type="KBC")
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, float(g["omega"]), int(g["steps"]))
    assert np.array_equal(f_0.numpy(), g["f"])


CASES = [
    # lattice, shape, policy, collision, omega, steps
    ("D3Q19", (32, 32, 32), "FP32FP32", "BGK", 1.7, 8),
    ("D3Q19", (6, 10, 18), "FP32FP32", "BGK", 1.2, 6),  # nz % 4 != 0 -> one cell per thread
    ("D3Q19", (5, 7, 4), "FP32FP32", "BGK", 1.0, 5),  # nz == VEC: both row ends in one thread
    ("D3Q19", (3, 3, 8), "FP64FP64", "BGK", 1.9, 5),
    ("D3Q19", (8, 8, 8), "FP32FP16", "BGK", 1.1, 5),
    ("D3Q19", (8, 8, 8), "FP64FP16", "BGK", 1.1, 5),
    ("D3Q19", (8, 12, 16), "FP64FP32", "BGK", 1.5, 5),
    ("D3Q27", (8, 8, 12), "FP32FP32", "BGK", 1.6, 5),
    ("D3Q27", (8, 8, 12), "FP32FP32", "KBC", 1.95, 5),
    ("D3Q27", (4, 6, 10), "FP64FP32", "KBC", 1.8, 5),
    ("D2Q9", (24, 36), "FP32FP32", "BGK", 1.4, 10),
    ("D2Q9", (20, 30), "FP64FP64", "KBC", 1.9, 10),
    ("D2Q9", (1, 8), "FP32FP32", "BGK", 1.0, 3),
]


@pytest.mark.parametrize("lattice,shape,policy,collision,omega,steps", CASES)
def test_periodic_step_vs_oracle(lattice, shape, policy, collision, omega, steps, exact_math):
    vs, pp = init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    grid = grid_factory(shape)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type=collision)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_np = orc.perturbed_init(shape, lat, policy, seed=7, amp_rho=0.02, amp_u=0.03)
    f_0.assign(f_np)
    f_0, f_1 = run_reference_loop(stepper, f_0, f_1, bc_mask, missing_mask, omega, steps)
    bm = np.zeros((1,) + shape, np.uint8)
    mm = np.zeros((lat.q,) + shape, bool)
    exp = orc.run(f_np, bm, mm, [], omega, lat, steps, policy, collision)
    out = f_0.numpy()
    assert out.dtype == exp.dtype
    tol = {"FP32FP32": TOL, "FP64FP32": TOL, "FP64FP64": 1e-12, "FP32FP16": 2e-3, "FP64FP16": 2e-3}[policy]
    assert np.abs(out.astype(np.float64) - exp.astype(np.float64)).max() <= tol
    assert np.array_equal(out, exp), f"not bit-exact: max ulp {max_ulp_diff(out, exp)}"


@pytest.mark.parametrize("vec", [1, 4])
@pytest.mark.parametrize("shape", [(12, 16, 20), (16, 16, 16)])
def test_all_bc_kinds_in_one_step_vs_oracle(shape, vec):
    """Every in-scope BC kind at once (incl. a moving halfway wall and an interior solid
    sphere), with list order != id order, on the vectorised and the scalar kernel."""
    vs, pp = init_hip("D3Q19")
    get_context().set_option("vec", vec)
    try:
        lat = orc.Lattice("D3Q19")
        grid = grid_factory(shape)
        box = grid.bounding_box_indices()
        box_ne = grid.bounding_box_indices(remove_edges=True)
        n = shape[0]
        g3 = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        sph = [a.tolist() for a in np.where(sum((g - s // 2) ** 2 for g, s in zip(g3, shape)) < (n // 4) ** 2)]
        b_lid = EquilibriumBC(rho=1.0, u=(0.02, 0.0, 0.0), indices=box_ne["top"])
        b_mov = HalfwayBounceBackBC(indices=box_ne["bottom"], prescribed_value=(0.0, 0.01, 0.0))
        b_fw = FullwayBounceBackBC(indices=box_ne["left"])
        b_dn = DoNothingBC(indices=box_ne["right"])
        b_sph = HalfwayBounceBackBC(indices=sph)
        b_hw = HalfwayBounceBackBC(indices=box_ne["front"])
        bcs = [b_sph, b_fw, b_lid, b_dn, b_mov, b_hw]
        obcs = [
            orc.BC(orc.KIND_HALFWAY_BB, b_sph.id, sph),
            orc.BC(orc.KIND_FULLWAY_BB, b_fw.id, box_ne["left"]),
            orc.BC(orc.KIND_EQUILIBRIUM, b_lid.id, box_ne["top"], rho=1.0, u=(0.02, 0.0, 0.0)),
            orc.BC(orc.KIND_DO_NOTHING, b_dn.id, box_ne["right"]),
            orc.BC(orc.KIND_HALFWAY_BB, b_mov.id, box_ne["bottom"], u_wall=(0.0, 0.01, 0.0)),
            orc.BC(orc.KIND_HALFWAY_BB, b_hw.id, box_ne["front"]),
        ]
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs, collision_type="BGK")
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        o_bm, o_mm = orc.build_masks(shape, lat, obcs)
        assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
        f_np = orc.perturbed_init(shape, lat, seed=11)
        f_0.assign(f_np)
        steps = 7
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.3, steps)
        exp = orc.run(f_np, o_bm, o_mm, obcs, 1.3, lat, steps)
        out = f_0.numpy()
        assert np.abs(out - exp).max() <= TOL
        assert np.array_equal(out, exp), f"not bit-exact: max ulp {max_ulp_diff(out, exp)}"
    finally:
        get_context().set_option("vec", 0)


# (lattice, policy, walls): ghost planes of 4-, 2- and 8-byte elements; the D3Q19 FP32FP32 cases keep the ids they had before the others came
GHOST_CASES = [pytest.param(la, po, w, id=w.__name__ + ("" if (la, po) == ("D3Q19", "FP32FP32") else f"-{la}-{po}"))
               for la, po in (("D3Q19", "FP32FP32"), ("D3Q19", "FP32FP16"), ("D3Q19", "FP64FP64"), ("D3Q27", "FP64FP32"))
               for w in (FullwayBounceBackBC, HalfwayBounceBackBC)]


@pytest.mark.parametrize("lattice,policy,walls_cls", GHOST_CASES)
def test_ghost_plane_protocol_single_rank(lattice, policy, walls_cls):
    """Fields with ghost x-planes + self ring exchange (the slab protocol on one rank) give the
    same bits as the plain periodic kernel, with and without interior/edge splitting — and all of them the oracle's."""
    results = []
    shape = (10, 8, 16)
    for cfg in (None, {"halo": 1}, {"halo": 2}):
        grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls, lattice=lattice, policy=policy, backend_config=cfg)
        assert grid.halo == (cfg or {}).get("halo", 0)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        f_np = orc.perturbed_init(shape, lat, policy, seed=3)
        f_0.assign(f_np)
        for overlap in (1, 0):
            get_context().set_option("overlap", overlap)
            f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.4, 3)
        get_context().set_option("overlap", 1)
        results.append(f_0.numpy())
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    exp = orc.run(f_np, o_bm, o_mm, obcs, 1.4, lat, 6, policy)
    assert results[0].dtype == exp.dtype
    assert np.array_equal(results[0], exp), f"not bit-exact: max ulp {max_ulp_diff(results[0], exp)}"


def test_stepper_argument_errors():
    vs, pp = init_hip("D3Q19")
    grid = grid_factory((8, 8, 8))
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    with pytest.raises(Exception, match="different fields"):
        stepper(f_0, f_0, bc_mask, missing_mask, 1.0, 0)
    wrong = grid.create_field(9)
    with pytest.raises(Exception, match="cardinality"):
        stepper(f_0, wrong, bc_mask, missing_mask, 1.0, 0)
    with pytest.raises(AssertionError):
        IncompressibleNavierStokesStepper(grid=grid, streaming_scheme="push")
    with pytest.raises(NotImplementedError):
        IncompressibleNavierStokesStepper(grid=grid, collision_type="KBC")  # D3Q19 has no KBC (kbc.py:65-66)


@pytest.mark.parametrize("shape", [(5, 8, 64), (3, 16, 128), (1, 8, 64), (2, 24, 64)])
@pytest.mark.parametrize("walls_cls", [None, FullwayBounceBackBC, HalfwayBounceBackBC])
@pytest.mark.parametrize("steps", [2, 4, 7, 9])
def test_two_step_fusion_matches_oracle(shape, walls_cls, steps):
    """xlbhip_run with fuse2=1 (two steps per pass through LDS, step2_kernel.hpp) gives the same bits as the
    oracle — and therefore as the single-step kernel — for every parity of the step count."""
    ctx_opts = {"fuse2": 2}  # 2 = also the boundary-condition variant (1, the default, fuses only BC-free steppers)
    if walls_cls is None:
        vs, pp = init_hip("D3Q19")
        lat = orc.Lattice("D3Q19")
        grid = grid_factory(shape)
        bcs, obcs = [], []
    else:
        grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls)
    ctx = get_context()
    try:
        for k, v in ctx_opts.items():
            ctx.set_option(k, v)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        f_np = orc.perturbed_init(shape, lat, seed=23)
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.6, steps)
        if obcs:
            o_bm, o_mm = orc.build_masks(shape, lat, obcs)
        else:
            o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
        exp = orc.run(f_np, o_bm, o_mm, obcs, 1.6, lat, steps)
        out = f_0.numpy()
        assert np.array_equal(out, exp), f"max ulp {max_ulp_diff(out, exp)}, max abs {np.abs(out - exp).max()}"
    finally:
        ctx.set_option("fuse2", 1)


@pytest.mark.parametrize("shape", [(5, 8, 64), (4, 16, 128), (7, 8, 64)])
@pytest.mark.parametrize("steps", [2, 3, 6])
def test_two_step_fusion_d3q27_periodic(shape, steps):
    """D3Q27 BGK fp32 through the two-step kernel (periodic boxes: the 54-plane lifetime-packed LDS ring has no room for
    the boundary-condition form): same bits as the oracle; a stepper with walls must stay on the single-step kernel."""
    vs, pp = init_hip("D3Q27")
    lat = orc.Lattice("D3Q27")
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        grid = grid_factory(shape)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[])
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_np = orc.perturbed_init(shape, lat, seed=31)
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.7, steps)
        o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
        assert np.array_equal(f_0.numpy(), orc.run(f_np, o_bm, o_mm, [], 1.7, lat, steps))
        grid, bcs, lat, obcs = hip_cavity_3d((4, 8, 64), FullwayBounceBackBC, lattice="D3Q27")
        st2 = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        g_0, g_1, bm, mm = st2.prepare_fields()
        assert not st2._native_stepper().step2_eligible(g_0, g_1, bm, mm)
    finally:
        ctx.set_option("fuse2", 1)


@pytest.mark.parametrize("shape", [(5, 8, 48), (4, 16, 96), (7, 24, 48)])
@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP32"])
@pytest.mark.parametrize("exact", [1, 0])
def test_two_step_fusion_d3q27_kbc_periodic(shape, policy, exact):
    """D3Q27 KBC through the two-step kernel ((8 x 48) tiles; f(t+1) sits in LDS in the fp32 STORE type, as it would in
    memory, so the fp64-compute policy pairs too — BASELINE configs[4]).  Bit-exact builds: the oracle's bits for even and
    odd step counts.  The default fast fp64 collision: the same bits as single steps of the same collision, and the oracle
    to rounding."""
    vs, pp = init_hip("D3Q27", policy)
    lat = orc.Lattice("D3Q27")
    ctx = get_context()
    f_np = orc.perturbed_init(shape, lat, policy, seed=37, amp_rho=0.02, amp_u=0.03)
    o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    try:
        ctx.set_option("exact_math", exact)
        for steps in (2, 5):
            outs = []
            for mode in (2, 0):
                ctx.set_option("fuse2", mode)
                grid = grid_factory(shape)
                stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[], collision_type="KBC")
                f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
                # (the bit-exact fp64 collision is not built into the two-step kernel: scratch)
                assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask) == (mode == 2 and not (exact and policy == "FP64FP32"))
                f_0.assign(f_np)
                f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.9, steps)
                outs.append(f_0.numpy())
            assert np.array_equal(outs[0], outs[1])
            exp = orc.run(f_np, o_bm, o_mm, [], 1.9, lat, steps, policy, "KBC")
            if exact:
                assert np.array_equal(outs[0], exp)
            else:
                assert np.abs(outs[0].astype(np.float64) - exp.astype(np.float64)).max() <= 1e-6
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("exact_math", 0)


@pytest.mark.parametrize("shape", [(20, 8, 64), (16, 16, 64), (6, 8, 64)])
@pytest.mark.parametrize("walls_cls", [None, FullwayBounceBackBC, HalfwayBounceBackBC])
@pytest.mark.parametrize("steps", [2, 5, 8])
def test_two_step_fusion_slab_protocol(shape, walls_cls, steps):
    """The two-step kernel on fields with TWO ghost planes per side (the multi-rank layout) with the depth-2 ring
    exchange onto the rank itself: interior launch overlapped with the exchange + two edge launches (nx >= 16), or one
    launch after the exchange — same bits as the oracle on the periodic domain.  The x-walls of the cavity sit on the
    slab faces, so boundary cells (halfway redirects, fullway swaps, the moving lid's corner cells) are evaluated on
    the ghost planes as well."""
    cfg = {"halo": 2}
    if walls_cls is None:
        vs, pp = init_hip("D3Q19")
        lat = orc.Lattice("D3Q19")
        grid = grid_factory(shape, backend_config=cfg)
        bcs, obcs = [], []
    else:
        grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls, backend_config=cfg)
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert f_0.halo == 2 and stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_np = orc.perturbed_init(shape, lat, seed=29)
        if obcs:
            o_bm, o_mm = orc.build_masks(shape, lat, obcs)
        else:
            o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
        exp = orc.run(f_np, o_bm, o_mm, obcs, 1.6, lat, steps)
        for overlap in (1, 0):
            ctx.set_option("overlap", overlap)
            f_0.assign(f_np)
            a, b = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.6, steps)
            out = a.numpy()
            assert np.array_equal(out, exp), f"overlap={overlap}: max ulp {max_ulp_diff(out, exp)}, max abs {np.abs(out - exp).max()}"
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("overlap", 1)


def test_empty_and_ragged_index_lists():
    """Edge cases of the index-based BCs: a BC whose index lists are EMPTY tags no cell (the run is the periodic one, bit for bit, the
    masks are the oracle's); index lists of unequal lengths are refused; indices outside the box are dropped."""
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    shape = (6, 8, 64)
    grid = grid_factory(shape)
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[FullwayBounceBackBC(indices=[[], [], []]), HalfwayBounceBackBC(indices=[[], [], []])])
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    # (the masker still marks the directions that enter through the faces of the box as missing — on cells that carry no BC, where
    # nothing reads them: indices_boundary_masker.py:96-99, 131-134)
    e_bm, e_mm = orc.build_masks(shape, lat, [orc.BC(orc.KIND_FULLWAY_BB, 1, [[], [], []]), orc.BC(orc.KIND_HALFWAY_BB, 2, [[], [], []])])
    assert not bc_mask.numpy().any() and not e_bm.any() and np.array_equal(missing_mask.numpy(), e_mm.astype(np.uint8))
    f_np = orc.perturbed_init(shape, lat, seed=59)
    f_0.assign(f_np)
    f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.3, 5)
    z1, zq = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    assert np.array_equal(f_0.numpy(), orc.run(f_np, z1, zq, [], 1.3, lat, 5))
    with pytest.raises(Exception):
        bad = FullwayBounceBackBC(indices=[[1, 2, 3], [1, 2], [1, 2, 3]])
        IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[bad]).prepare_fields()
    # an index outside the box is dropped, like an out-of-bounds scatter update in the reference's JAX masker (indices_boundary_masker.py:128)
    out = FullwayBounceBackBC(indices=[[1, 2], [1, 3], [64, 5]])  # z = 64 is outside; (2, 3, 5) is a cell
    _, _, bm2, _ = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[out]).prepare_fields()
    tagged = np.argwhere(bm2.numpy()[0] == out.id)
    assert tagged.tolist() == [[2, 3, 5]]


@pytest.mark.parametrize("walls_cls", [HalfwayBounceBackBC, FullwayBounceBackBC])
@pytest.mark.parametrize("steps", [4, 5])
def test_two_step_clean_items_on_the_slack_ring(walls_cls, steps):
    """A lid-driven cavity cut into thin end segments and clean middle segments (fuse2_xseg = 4 at nx = 48: planes 0-8, 8-24, 24-40,
    40-48): the middle segments of the interior tile columns carry no boundary cell and run the BC-free body on its slack LDS ring
    (one barrier per plane) inside the BC kernel, next to hull items on the 43-plane ring — bit for bit against the oracle, and the
    same with the clean flags off."""
    shape, omega = (48, 24, 192), 1.4
    grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls)
    ctx = get_context()
    f_np = orc.perturbed_init(shape, lat, seed=41)
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    exp = orc.run(f_np, o_bm, o_mm, obcs, omega, lat, steps)
    try:
        ctx.set_option("fuse2", 2)
        ctx.set_option("fuse2_xseg", 4)
        for clean in (1, 0):
            ctx.set_option("fuse2_clean", clean)
            if clean == 0:  # (a stepper consumes the index lists of its BC objects, as the reference's does: fresh ones for the second)
                grid, bcs, _, _ = hip_cavity_3d(shape, walls_cls)
            stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
            f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
            assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
            f_0.assign(f_np)
            f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, steps)
            out = f_0.numpy()
            assert np.array_equal(out, exp), f"fuse2_clean={clean}: max abs {np.abs(out - exp).max()}"
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("fuse2_xseg", 0)
        ctx.set_option("fuse2_clean", 1)


@pytest.mark.parametrize("faces", [("front", "back"), ("front",), ("bottom", "top")])
def test_two_step_y_wall_redirect_regression(faces):
    """Regression for the memory fault of round 1 (gpurun_out/f.err, fixed by commit 2111f4e): halfway walls on the y
    faces make EVERY wave of a hull tile issue the redirected own-cell loads of the two-step kernel — inline-asm
    `global_load_dword v, v_off, s[base]` whose SGPR base may have just been written by a VALU (v_readlane of a spilled
    SGPR); without the `s_nop 4` in front the load used a garbage address.  A domain whose only boundary is a pair of
    y (or z) walls, several tiles and x-segments, bit for bit against the oracle."""
    vs, pp = init_hip("D3Q19")
    lat = orc.Lattice("D3Q19")
    shape, omega, steps = (40, 32, 128), 1.3, 4
    grid = grid_factory(shape)
    box = grid.bounding_box_indices()
    walls = [sum((box[f][i] for f in faces), []) for i in range(3)]
    bc = HalfwayBounceBackBC(indices=walls)
    obcs = [orc.BC(orc.KIND_HALFWAY_BB, bc.id, walls)]
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        ctx.set_option("fuse2_xseg", 4)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=[bc])
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_np = orc.perturbed_init(shape, lat, seed=37)
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, steps)
        o_bm, o_mm = orc.build_masks(shape, lat, obcs)
        assert np.array_equal(f_0.numpy(), orc.run(f_np, o_bm, o_mm, obcs, omega, lat, steps))
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("fuse2_xseg", 0)


@pytest.mark.parametrize("walls_cls", [None, HalfwayBounceBackBC, FullwayBounceBackBC])
@pytest.mark.parametrize("halo", [0, 2])
def test_two_step_strip_buffers_follow_the_fields(walls_cls, halo):
    """Strip buffers of the two-step kernel (step2_kernel.hpp; round 3): phase A takes the halo columns of its grown tile from
    the source field's strips, phase B writes the destination's.  The strips are a cache of the field: whatever else writes
    a field must invalidate them.  One scenario exercises every way in — a first pass that only writes strips (its source has none yet),
    strips written by phase B and re-read, a single step in between (k_step writes the field, not its strips), a host upload
    into a field whose strips were valid, a run with the strips switched off and on again, the wide (nz = 128: two tile
    columns, so the halo columns really come from ANOTHER tile's cells) and the slab layout — against the oracle, bit for bit."""
    shape = (20, 16, 128)
    cfg = {"halo": halo} if halo else None
    if walls_cls is None:
        vs, pp = init_hip("D3Q19")
        lat = orc.Lattice("D3Q19")
        grid = grid_factory(shape, backend_config=cfg)
        bcs, obcs = [], []
        o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    else:
        grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls, backend_config=cfg)
        o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        assert ctx.get_option("fuse2_strips") == 1  # the default: strips for steppers with boundary conditions
        ctx.set_option("fuse2_strips", 2)           # here: for the periodic box too
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_np = orc.perturbed_init(shape, lat, seed=41)
        f_0.assign(f_np)
        state = f_np
        # 7 steps: strips built from f_0, written by three passes and re-read, then one single step
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 7)
        state = orc.run(state, o_bm, o_mm, obcs, 1.5, lat, 7)
        assert np.array_equal(f_0.numpy(), state)
        # the single step left a field whose strips are stale: the next pairs must rebuild them
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 4)
        state = orc.run(state, o_bm, o_mm, obcs, 1.5, lat, 4)
        assert np.array_equal(f_0.numpy(), state)
        # a host upload into a field with valid strips
        state = orc.perturbed_init(shape, lat, seed=43)
        f_0.assign(state)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 2)
        state = orc.run(state, o_bm, o_mm, obcs, 1.5, lat, 2)
        assert np.array_equal(f_0.numpy(), state)
        # strips off for a run (the fields change, their strips do not), then on again
        ctx.set_option("fuse2_strips", 0)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 2)
        ctx.set_option("fuse2_strips", 2)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 4)
        state = orc.run(state, o_bm, o_mm, obcs, 1.5, lat, 6)
        assert np.array_equal(f_0.numpy(), state)
        # the measurement variant: row-aligned lanes in the bodies of the BC kernel, no strips
        ctx.set_option("fuse2_strips", 0)
        ctx.set_option("fuse2_rowmap", 1)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.5, 4)
        state = orc.run(state, o_bm, o_mm, obcs, 1.5, lat, 4)
        assert np.array_equal(f_0.numpy(), state)
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("fuse2_strips", 1)
        ctx.set_option("fuse2_rowmap", 0)


@pytest.mark.parametrize("shape", [(6, 8, 48), (7, 16, 96), (20, 24, 48)])
@pytest.mark.parametrize("walls_cls", [HalfwayBounceBackBC, FullwayBounceBackBC])
@pytest.mark.parametrize("steps", [2, 5])
def test_two_step_fusion_d3q27_with_walls(shape, walls_cls, steps):
    """Round 3 (VERDICT r02 "missing" 2): D3Q27 BGK fp32 WITH the basic boundary conditions through the two-step kernel — the
    63-plane BC ring on (8 x 48) tiles, the "wide" meta word (3 + 3 + 26 bits: 27 populations do not fit the D3Q19 layout),
    27 counted stores behind the redirected loads.  Lid-driven cavity with halfway or fullway walls: the oracle's bits."""
    grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls, lattice="D3Q27")
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_np = orc.perturbed_init(shape, lat, seed=61)
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.6, steps)
        o_bm, o_mm = orc.build_masks(shape, lat, obcs)
        exp = orc.run(f_np, o_bm, o_mm, obcs, 1.6, lat, steps)
        out = f_0.numpy()
        assert np.array_equal(out, exp), f"max ulp {max_ulp_diff(out, exp)}, max abs {np.abs(out - exp).max()}"
    finally:
        ctx.set_option("fuse2", 1)


def test_automatic_choice_keeps_d3q27_with_walls_on_single_steps():
    """fuse2 = 1 (the default) must not pick the D3Q27-with-BCs two-step kernel: it is 20-45 % slower than single steps
    (profiles/r03/d3q27_walls_two_step.md).  A rule that a later edit of can_fuse2 once dropped silently."""
    grid, bcs, lat, obcs = hip_cavity_3d((128, 384, 384), HalfwayBounceBackBC, lattice="D3Q27")  # (fills the chip: no other rule of fuse2 = 1 refuses it)
    ctx = get_context()
    assert ctx.get_option("fuse2") == 1
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    assert not stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
    try:
        ctx.set_option("fuse2", 2)
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
    finally:
        ctx.set_option("fuse2", 1)


def test_two_step_fusion_d3q27_all_basic_kinds():
    """... and every kind the two-step kernel evaluates at once — equilibrium lid, fullway wall, resting and MOVING halfway walls
    (the moving one is a kind of its own inside the wide meta word), an interior solid sphere (whose cells carry missing bit 0,
    which the wide word drops) — list order != id order, odd step count."""
    shape = (14, 16, 48)
    vs, pp = init_hip("D3Q27")
    lat = orc.Lattice("D3Q27")
    grid = grid_factory(shape)
    box_ne = grid.bounding_box_indices(remove_edges=True)
    g3 = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    sph = [a.tolist() for a in np.where(sum((g - s // 2) ** 2 for g, s in zip(g3, shape)) < 3.2**2)]
    b_lid = EquilibriumBC(rho=1.0, u=(0.02, 0.0, 0.0), indices=box_ne["top"])
    b_mov = HalfwayBounceBackBC(indices=box_ne["bottom"], prescribed_value=(0.0, 0.01, 0.0))
    b_fw = FullwayBounceBackBC(indices=box_ne["left"])
    b_sph = HalfwayBounceBackBC(indices=sph)
    b_hw = HalfwayBounceBackBC(indices=box_ne["front"])
    bcs = [b_sph, b_fw, b_lid, b_mov, b_hw]
    obcs = [orc.BC(orc.KIND_HALFWAY_BB, b_sph.id, sph), orc.BC(orc.KIND_FULLWAY_BB, b_fw.id, box_ne["left"]),
            orc.BC(orc.KIND_EQUILIBRIUM, b_lid.id, box_ne["top"], rho=1.0, u=(0.02, 0.0, 0.0)),
            orc.BC(orc.KIND_HALFWAY_BB, b_mov.id, box_ne["bottom"], u_wall=(0.0, 0.01, 0.0)), orc.BC(orc.KIND_HALFWAY_BB, b_hw.id, box_ne["front"])]
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        o_bm, o_mm = orc.build_masks(shape, lat, obcs)
        assert np.array_equal(bc_mask.numpy(), o_bm) and np.array_equal(missing_mask.numpy(), o_mm.astype(np.uint8))
        f_np = orc.perturbed_init(shape, lat, seed=67)
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, 1.3, 7)
        assert np.array_equal(f_0.numpy(), orc.run(f_np, o_bm, o_mm, obcs, 1.3, lat, 7))
    finally:
        ctx.set_option("fuse2", 1)
