"""examples/droplet_on_wall_2d_hip.py runs end to end at 96 x 40: the base width of the sessile droplet rises with the wall density
(the ordering the restatement shows in tests/test_multiphase_ref.py) and the fields end finite."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_base_width_rises_with_the_wall_density(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "droplet_on_wall_2d_hip.py"), "--nx", "96", "--ny", "40", "--wall-density", "0.8", "1.2",
                          "1.8"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    rows = re.findall(r"wall density ([0-9.]+): base width (\d+), height (\d+),.*fields finite: (True|False)", res.stdout)
    assert [r[0] for r in rows] == ["0.8", "1.2", "1.8"] and all(r[3] == "True" for r in rows)
    base = [int(r[1]) for r in rows]
    assert 0 < base[0] < base[1] < base[2], base
