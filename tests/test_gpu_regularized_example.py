"""examples/double_shear_layer_2d_hip.py runs end to end at 64 x 64: BGK is lost on the way, both regularised collisions end finite with
max |u| < 0.1 (fp64 NumPy: 0.059-0.062; profiles/regularized_collision.md)."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_double_shear_layer_example(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "double_shear_layer_2d_hip.py"), "--n", "64"], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    assert re.search(r"^BGK: lost by step \d+", res.stdout, re.M)
    for form in ("RegularizedBGK", "RecursiveRegularizedBGK"):
        m = re.search(rf"^{form}: finite after 3200 steps, max \|u\| = ([0-9.]+)", res.stdout, re.M)
        assert m and float(m.group(1)) < 0.1, res.stdout
    assert "regularised runs survive: True; BGK lost: True" in res.stdout
