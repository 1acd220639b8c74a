"""examples/obstacle_identification_hip.py at a small size, on the device and with ``--reference`` (the same loop through the NumPy
restatement on the host): the two print the same loss sequence, and the loss falls.

The size (64 x 24, 40 steps, 8 iterations) was chosen on the host through the restatement: every iteration is accepted at the first or
second trial step and the loss falls in each.  The device computes the bits of the restatement, so the two loops take the same steps; a
loss is a sum of N = d n_cells squares formed on the host in one order from fields that may differ in the order of the sums behind them
only, hence the bound N 2^-52 loss."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = ["--nx", "64", "--ny", "24", "--steps", "40", "--iterations", "8"]


def run(tmp_path, *extra):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "obstacle_identification_hip.py"), *SIZE, *extra], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    losses = [float(v) for v in re.findall(r"iteration \d+: loss = ([-0-9.eE+]+)", res.stdout)]
    final, first = (float(v) for v in re.search(r"final loss = ([-0-9.eE+]+) \(first ([-0-9.eE+]+)\)", res.stdout).groups())
    distance = float(re.search(r"final \|alpha - hidden\| = ([0-9.]+)", res.stdout).group(1))
    return losses, final, first, distance


def test_obstacle_identification_matches_the_reference_loop_and_descends(tmp_path):
    losses, final, first, distance = run(tmp_path)
    losses_ref, final_ref, _, distance_ref = run(tmp_path, "--reference")
    assert len(losses) == len(losses_ref) == 8
    n_terms = 2 * 64 * 24
    for a, b in zip(losses + [final], losses_ref + [final_ref]):
        assert abs(a - b) <= n_terms * 2.0**-52 * abs(b), f"loss {a!r} on the device, {b!r} through the restatement"
    assert all(b < a for a, b in zip(losses, losses[1:])), f"the loss did not fall: {losses}"
    assert final < first
    print(f"loss reduced by a factor {first / final:.2f}; |alpha - hidden| = {distance:.6f} (restatement: {distance_ref:.6f})")
