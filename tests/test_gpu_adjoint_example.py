"""examples/viscosity_identification_hip.py runs end to end for its default handful of iterations: the loss never increases from one
printed iteration to the next, and the final omega is closer to the target than the starting omega was."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_viscosity_identification_descends_towards_the_target(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "viscosity_identification_hip.py")], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    losses = [float(v) for v in re.findall(r"loss = ([-0-9.eE+]+)", res.stdout)]
    assert len(losses) >= 5
    assert all(b <= a for a, b in zip(losses, losses[1:])), f"the loss increased: {losses}"
    final, target, start = (float(v) for v in re.search(r"final omega = ([0-9.]+) \(target ([0-9.]+), started at ([0-9.]+)\)", res.stdout).groups())
    assert abs(final - target) < abs(start - target)
