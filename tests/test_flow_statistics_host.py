"""FlowStatistics without a GPU: the host-compilable half of xlb_amd/csrc/stats_kernels.hpp (the channels of one cell, the cell -> bin
map, the item -> cells plan) is compiled with clang++ through tests/hip_on_cpu, run cell by cell in the plan's order by
tests/stats_cpu_emulation.cpp and compared with the NumPy restatement tests/_stats_ref.py at the derived bound 2 n 2^-53 sum|x| per bin
and channel (counts, non-finite counts and the largest u.u: exactly).  Also: the plan's properties, the operator's argument checks
and the arithmetic of result() / reynolds_stress().  The GPU's code generation and wave shuffles are tests/test_gpu_flow_statistics.py's."""

import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import xlb_amd
from oracle import xlb_numpy as orc
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.operator.postprocess import FlowStatistics
from xlb_amd.operator.postprocess.flow_statistics import channel_names, means_from_sums, reynolds_stress_from_means

import _stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"D3Q19": (37, 22, 70), "D3Q27": (37, 22, 70), "D2Q9": (45, 70)}
KEEPS_3D = [(), (2,), (0,), (0, 2), (1, 2), (0, 1, 2)]
KEEPS_2D = [(), (1,), (0,), (0, 1)]
CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.float16): 2}
LATTICE_ID = {"D2Q9": 0, "D3Q19": 1, "D3Q27": 2}


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("stats_cpu") / "libstats_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "stats_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=900)
    lib = C.CDLL(str(so))
    lib.stats_sample_cpu.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 5 + [C.c_void_p] * 3
    lib.stats_plan_cpu.argtypes = [C.c_int] * 4 + [C.c_void_p]
    lib.stats_visit_cpu.argtypes = [C.c_int] * 5 + [C.c_int64] + [C.c_void_p] * 3
    lib.stats_visit_cpu.restype = C.c_int64
    return lib


def storage3(shape):
    return (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)


def keep_mask(keep_axes, dim):
    return sum(1 << (a + 3 - dim) for a in keep_axes)


class Emulated:
    """Running sums of the emulation, fed with host arrays in the reference layout (q, *shape); ``halo`` ghost planes full of NaN are put
    around the field first (they must never be read into a sum)."""

    def __init__(self, lib, lattice, policy, shape, keep_axes, order=2, exclude_ids=(255,), halo=0):
        self.lib, self.lattice, self.policy, self.shape, self.halo, self.order = lib, lattice, policy, tuple(shape), halo, order
        self.keep = keep_mask(keep_axes, len(shape))
        self.bins_shape = tuple(shape[a] for a in sorted(keep_axes))
        self.channels = ref.channel_count(len(shape), order)
        self.sums = np.zeros((self.channels,) + self.bins_shape)
        self.exclude = np.zeros(8, np.uint32)
        for v in exclude_ids:
            self.exclude[v >> 5] |= np.uint32(1 << (v & 31))
        self.watch = np.zeros(2, np.uint64)

    def _with_ghosts(self, a, fill):
        nx, ny, nz = storage3(self.shape)
        a = a.reshape((a.shape[0], nx, ny, nz))
        out = np.full((a.shape[0], nx + 2 * self.halo, ny, nz), fill, a.dtype)
        out[:, self.halo : self.halo + nx] = a
        return out

    def sample(self, f, bc_mask=None):
        S, T = orc.store_dtype(self.policy), orc.compute_dtype(self.policy)
        nx, ny, nz = storage3(self.shape)
        fs = np.ascontiguousarray(self._with_ghosts(np.asarray(f).astype(S), np.nan))
        bm = None if bc_mask is None else np.ascontiguousarray(self._with_ghosts(np.asarray(bc_mask).astype(np.uint8), 0))
        self.watch[:] = 0
        got = self.lib.stats_sample_cpu(LATTICE_ID[self.lattice], CODE[np.dtype(T)], CODE[np.dtype(S)], fs.ctypes.data, fs[0].size, self.halo,
                                        None if bm is None else bm.ctypes.data, self.halo, nx, ny, nz, self.keep, self.order, self.exclude.ctypes.data,
                                        self.sums.ctypes.data, self.watch.ctypes.data)
        assert got == self.channels
        bits = int(self.watch[0])
        self.max_u2 = float(np.array([bits], np.uint64).view(np.float64)[0]) if T == np.float64 else float(np.array([bits], np.uint32).view(np.float32)[0])
        self.nonfinite = int(self.watch[1])


def flow(lattice, policy, steps=3, seed=3):
    lat = orc.Lattice(lattice)
    shape = SHAPES[lattice]
    f = orc.perturbed_init(shape, lat, policy, seed=seed)
    bm, mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    for _ in range(steps):
        f = orc.step(f, bm, mm, [], 1.3, lat, policy, "BGK")
    return lat, shape, f


def random_mask(shape, seed=11):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0, 0, 1, 7, 255], np.uint8), size=(1,) + tuple(shape))


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64", "FP32FP16"])
@pytest.mark.parametrize("lattice", ["D2Q9", "D3Q19", "D3Q27"])
def test_emulated_kernels_match_the_restatement(emulation, lattice, policy):
    lat, shape, f = flow(lattice, policy)
    bm = random_mask(shape)
    for keep in KEEPS_2D if lat.d == 2 else KEEPS_3D:
        for mask, exclude in ((None, (255,)), (bm, (7, 255))):
            e = Emulated(emulation, lattice, policy, shape, keep, exclude_ids=exclude)
            e.sample(f, mask)
            r = ref.restate(f, lat, policy, keep, 2, mask, exclude)
            ref.assert_sums_match(e.sums, r, f"{lattice} {policy} keep {keep} mask {mask is not None}")
            assert e.max_u2 == r["max_u2"] and e.nonfinite == r["nonfinite"] == 0
            if mask is not None:
                assert e.sums[0].sum() == np.count_nonzero(~np.isin(bm, exclude))


def test_order_1_accumulation_over_samples_and_non_finite_cells(emulation):
    lat, shape, f = flow("D3Q19", "FP32FP32")
    bm = random_mask(shape)
    bad = f.copy()
    cells = [(3, 4, 5), (36, 21, 69), (0, 0, 64)]
    bm[(0,) + cells[0]] = bm[(0,) + cells[1]] = bm[(0,) + cells[2]] = 0
    bad[5][cells[0]] = np.nan
    bad[0][cells[1]] = np.inf
    bad[:, cells[2][0], cells[2][1], cells[2][2]] = 0.0  # rho = 0: u = 0 / 0
    excluded = tuple(np.argwhere(bm[0] == 255)[0])
    bad[2][excluded] = np.nan
    e = Emulated(emulation, "D3Q19", "FP32FP32", shape, (2,), order=1)
    total = None
    for sample in (f, bad, f):
        e.sample(sample, bm)
        total = ref.accumulate(total, ref.restate(sample, lat, "FP32FP32", (2,), 1, bm))
    ref.assert_sums_match(e.sums, total, "order 1, three samples")
    assert e.sums.shape[0] == 5 and total["nonfinite_total"] == 3 and e.nonfinite == 0
    e.sample(bad, bm)
    r = ref.restate(bad, lat, "FP32FP32", (2,), 1, bm)
    assert e.nonfinite == r["nonfinite"] == 3 and e.max_u2 == r["max_u2"] and np.isfinite(e.sums).all()


@pytest.mark.parametrize("shape3", [(37, 22, 70), (1, 45, 70), (64, 64, 128), (5, 3, 2), (300, 7, 65)])
def test_every_cell_is_in_exactly_one_partial_whatever_the_ghost_planes(emulation, shape3):
    nx, ny, nz = shape3
    cells = nx * ny * nz
    for keep in range(8):
        plan = np.zeros(7, np.int64)
        emulation.stats_plan_cpu(nx, ny, nz, keep, plan.ctypes.data)
        nk, ns, nzc, ch, nj, items, bins = (int(v) for v in plan)
        assert nj == -(-ns // ch) and items == nk * nj * (nzc if keep & 4 else 1)
        assert bins == (nx if keep & 1 else 1) * (ny if keep & 2 else 1) * (nz if keep & 4 else 1)
        # the scratch bound of DESIGN.md: partials only while there are fewer than 4096 items per chunk, never more than 2 x 4096 x 64 of them
        assert nj == 1 or nj * bins <= 2 * 4096 * 64
        seen = None
        for halo in (0, 1, 2):
            cell, part, bin_ = (np.zeros(cells + 1, np.int64) for _ in range(3))
            n = emulation.stats_visit_cpu(nx, ny, nz, keep, halo, cells + 1, cell.ctypes.data, part.ctypes.data, bin_.ctypes.data)
            assert n == cells
            interior = cell[:n] - halo * ny * nz  # storage index -> index without ghost planes
            assert interior.min() >= 0 and interior.max() < cells and np.array_equal(np.sort(interior), np.arange(cells))  # each exactly once, no ghost
            x, y, z = np.unravel_index(interior, shape3)
            expect = ((x if keep & 1 else 0) * (ny if keep & 2 else 1) + (y if keep & 2 else 0)) * (nz if keep & 4 else 1) + (z if keep & 4 else 0)
            assert np.array_equal(bin_[:n], np.broadcast_to(expect, (n,))) and part[:n].max() == nj - 1
            this = (interior, part[:n].copy(), bin_[:n].copy())
            if seen is not None:
                assert all(np.array_equal(a, b) for a, b in zip(seen, this)), "the plan depends on the ghost planes"
            seen = this


def test_ghost_planes_are_never_sampled_and_change_no_bit(emulation):
    lat, shape, f = flow("D3Q27", "FP64FP64")
    bm = random_mask(shape)
    for keep in ((), (2,), (0,)):
        runs = []
        for halo in (0, 1, 2):
            e = Emulated(emulation, "D3Q27", "FP64FP64", shape, keep, halo=halo)  # ghost planes hold NaN
            e.sample(f, bm)
            runs.append(e.sums.copy())
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def fake_grid(shape):
    return types.SimpleNamespace(shape=tuple(shape), local_shape=tuple(shape), halo=0, n_ranks=1, x_offset=0)


def make(shape, lattice="D3Q19", **kw):
    pp = PrecisionPolicy.FP32FP32
    vs = getattr(xlb_amd.velocity_set, lattice)(pp, ComputeBackend.HIP)
    return FlowStatistics(fake_grid(shape), velocity_set=vs, precision_policy=pp, compute_backend=ComputeBackend.HIP, **kw)


def test_argument_checks_name_the_problem():
    s = make((8, 6, 4), keep_axes=(2, 0))
    assert s.keep_axes == (0, 2) and s.bins_shape == (8, 4) and s._keep_mask == 5 and len(s.channels) == 12 and s.samples == 0
    s2 = make((9, 5), "D2Q9", keep_axes=(1,), order=1)
    assert s2._shape3 == (1, 9, 5) and s2._keep_mask == 4 and s2.bins_shape == (5,) and s2.channels == ["count", "rho", "ux", "uy"]
    with pytest.raises(ValueError, match="twice"):
        make((8, 6, 4), keep_axes=(2, 2))
    with pytest.raises(ValueError, match="out of range"):
        make((8, 6, 4), keep_axes=(3,))
    with pytest.raises(ValueError, match="out of range"):
        make((8, 6), "D2Q9", keep_axes=(2,))
    with pytest.raises(ValueError, match="order"):
        make((8, 6, 4), order=3)
    with pytest.raises(ValueError, match="2-D grid with the 3-D lattice"):
        make((8, 6), "D3Q19")
    with pytest.raises(ValueError, match="exclude_ids"):
        make((8, 6, 4), exclude_ids=(256,))
    with pytest.raises(ValueError, match="population field"):
        s._check_fields(np.zeros((19, 8, 6, 4), np.float32), None)


def test_result_and_reynolds_stress_arithmetic():
    rng = np.random.default_rng(2)
    d, bins, samples = 3, 5, 4
    n = np.array([10.0, 12.0, 0.0, 7.0, 9.0]) * samples
    sums = rng.normal(size=(12, bins)) * n
    sums[0] = n
    r = means_from_sums(sums, samples, d, 2)
    assert np.array_equal(r["count"], n / samples) and r["sums"] is not None and r["u"].shape == (3, bins) and r["uu"].shape == (6, bins)
    ok = n > 0
    n = np.where(ok, n, 1.0)  # (what is compared below is compared where there are cells)
    assert np.array_equal(r["rho"][ok], (sums[1] / n)[ok]) and np.isnan(r["rho"][~ok]).all()
    assert np.array_equal(r["rho2"][ok], (sums[2] / n)[ok]) and np.array_equal(r["u"][:, ok], (sums[3:6] / n)[:, ok])
    rs = reynolds_stress_from_means(r["u"], r["uu"])
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for k, (a, b) in enumerate(pairs):
        assert np.array_equal(rs[k][ok], (sums[6 + k] / n - sums[3 + a] / n * (sums[3 + b] / n))[ok])
    assert channel_names(3, 2)[6:] == ["uxux", "uxuy", "uxuz", "uyuy", "uyuz", "uzuz"] and channel_names(2, 2) == ["count", "rho", "rho2", "ux", "uy", "uxux", "uxuy", "uyuy"]
    r1 = means_from_sums(sums[:5], samples, d, 1)
    assert "uu" not in r1 and np.array_equal(r1["u"][:, ok], (sums[2:5] / n)[:, ok])
    with pytest.raises(ValueError, match="channels"):
        means_from_sums(sums[:7], samples, d, 2)
    s = make((8, 6, 4), keep_axes=(2,), order=1)
    with pytest.raises(ValueError, match="order=2"):
        s.reynolds_stress()
    # an operator that never sampled reads nothing from a device
    empty = make((8, 6, 4), keep_axes=(2,)).result()
    assert empty["samples"] == 0 and empty["sums"].shape == (12, 4) and not empty["sums"].any()
