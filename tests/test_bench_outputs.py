"""bench.py's plain line, its --full additions and --dump-outputs: the dumped populations are what the timed path computed."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_cells_every_cell_or_a_fixed_sample_within_budget():
    shape, row = (16, 16, 16), 19 * 4 + 8
    assert np.array_equal(bench.dump_cells(shape, row), np.arange(16**3))
    shape = (512, 512, 512)
    a, b = bench.dump_cells(shape, row), bench.dump_cells(shape, row)
    assert np.array_equal(a, b)  # the same cells in every run
    assert a.size * row <= bench.DUMP_BYTES < (a.size + 1) * row
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 512**3
    assert a.max() > 0.99 * 512**3 and a.min() < 0.01 * 512**3  # spread over the whole box
    assert bench.DUMP_BYTES + 2 * 256 < 64_000_000  # with two .npy headers


def test_plain_run_is_lean_by_default():
    args = bench.parse(["--steps", "7"])
    assert args.steps == 7 and args.full is False and args.dump_outputs == ""
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True


def _bench(tmp_path, *extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *extra], cwd=tmp_path, capture_output=True, text=True,
                         timeout=600, env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 128])
def test_dumped_outputs_equal_the_c_oracle(tmp_path, n):
    """32^3: every cell is written; 128^3 (160 MB of populations): the fixed sample.  Both bit-identical to oracle/lbm_ref.c after
    warm-up + timed steps from the same start."""
    from oracle import lbm_ref, xlb_numpy as orc

    warmup, steps = 3, 5
    rec = _bench(tmp_path, "--size", str(n), "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out"))
    assert rec["steps"] == steps and rec["warmup"] == warmup and rec["ms_per_step"] > 0 and rec["unit"] == "MLUPS"
    assert "cpu_baseline" not in rec and rec["roofline"]["copy_yardstick_gbs"] is None and rec["roofline"]["pattern_copy_ms"] is None
    assert sorted(os.listdir(tmp_path / "out")) == ["f_0.npy", "f_0_cells.npy"]
    rows = np.load(tmp_path / "out" / "f_0.npy")
    cells = np.load(tmp_path / "out" / "f_0_cells.npy")
    assert rows.dtype == np.float32 and cells.dtype == np.float64 and rows.shape == (cells.size, 19)
    assert np.array_equal(cells, bench.dump_cells((n, n, n), 19 * 4 + 8).astype(np.float64))
    assert (cells.size == n**3) == (n == 32)

    lat, shape, obcs = orc.cavity_3d(n, orc.KIND_HALFWAY_BB)
    o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    exp = lbm_ref.run(orc.initialize_eq(shape, lat), o_bm, o_mm, obcs, 1.0, lat, warmup + steps)
    exp = exp.reshape(19, -1)[:, cells.astype(np.int64)].T
    assert np.array_equal(rows, exp)
    assert float(np.abs(rows - rows[:1]).max()) > 1e-4  # the lid has moved something


@pytest.mark.gpu
def test_full_adds_the_yardsticks_and_the_cpu_baseline(tmp_path):
    rec = _bench(tmp_path, "--size", "64", "--steps", "4", "--warmup", "2", "--full", "--cpu-baseline-seconds", "1", "--cpu-baseline-size", "32")
    assert rec["steps"] == 4 and rec["ms_per_step"] > 0
    assert rec["roofline"]["copy_yardstick_gbs"] > 0
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["legs"]
