"""examples/droplet_in_fluid_2d_hip.py runs end to end at a reduced size (48 x 48, radius 11, 2000 steps): both masses stay where they
were, Laplace's product is positive and the fields end finite."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_droplet_keeps_both_masses_and_has_a_positive_laplace_product(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "droplet_in_fluid_2d_hip.py"), "--n", "48", "--radius", "11", "--steps", "2000"],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    masses = re.findall(r"mass of ([AB]): ([0-9.]+) -> ([0-9.]+)", res.stdout)
    assert [m[0] for m in masses] == ["A", "B"]
    for _, before, after in masses:
        # (the sums are printed with six decimals: the scheme's own drift is nine orders below, tests/test_multicomponent_ref.py)
        assert abs(float(after) - float(before)) <= 2e-6, masses
    product = re.search(r"Laplace product \(p_in - p_out\) R = ([-0-9.]+), fields finite: (True|False)", res.stdout)
    assert product and product.group(2) == "True"
    assert float(product.group(1)) > 0.0, product.group(1)  # (about 0.15 when relaxed: profiles/multicomponent.md)
    radius = float(re.search(r"R = ([0-9.]+),", res.stdout).group(1))
    assert 8.0 < radius < 14.0
