"""examples/rayleigh_benard_2d_hip.py runs end to end at a small size: above the critical Rayleigh number (1708) the layer convects —
Nu > 1 — and the fields end finite; below it the layer conducts.  No quantitative Nusselt number is claimed."""

import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_example(tmp_path, *args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "rayleigh_benard_2d_hip.py"), "--nx", "64", "--ny", "32"] + list(args),
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "fields finite: True" in res.stdout
    return float(re.search(r"Nu = ([-0-9.eE+]+)", res.stdout).group(1))


def test_rayleigh_benard_convects_above_the_critical_rayleigh_number(tmp_path):
    assert run_example(tmp_path, "--ra", "2e4", "--expect-convection") > 1.0


def test_rayleigh_benard_conducts_below_it(tmp_path):
    """Below the critical Rayleigh number the perturbation decays and the layer conducts: Nu = 1 exactly in the continuum, and the
    linear profile is an exact solution of the scheme (tests/test_scalar_ref.py), so what is left after 60 free-fall times is the
    decaying roll; 5 % tells conduction from convection (Nu = 3.2 at Ra = 2e4) with a wide margin on both sides."""
    nusselt = run_example(tmp_path, "--ra", "800")
    print("Nu below the critical Rayleigh number:", nusselt)
    assert abs(nusselt - 1.0) < 0.05
