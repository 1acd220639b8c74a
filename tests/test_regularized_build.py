"""No-spill guard of the regularised collisions' D3Q19 unit: the collision is meant to hide under the single-step kernel's HBM traffic,
which it cannot do from scratch memory.  Compiles xlb_amd/csrc/step_d3q19_reg.hip to gfx950 assembly (needs hipcc, no GPU)."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_listing(tmp_path_factory, unit):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp(unit) / (unit + ".s")
    # (the Makefile's flags for this unit: REGFLAGS)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm", "-pragma-unroll-threshold=200000", "-mllvm", "-split-spill-mode=size",
           f"-I{os.path.join(ROOT, 'include')}", "-S", "--cuda-device-only",
           "-o", str(out), os.path.join(ROOT, "xlb_amd", "csrc", unit + ".hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    # the metadata lists, per kernel, .name ... .private_segment_fixed_size ... .vgpr_count; k_step<D3Q19, float, float, ...> mangles to ...D3Q19Eff...
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s*(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s*(\d+)", out.read_text())
    return [(name, int(size), int(vgprs)) for name, size, vgprs in kernels if "k_step" in name and "5D3Q19EffLi" in name]


@pytest.fixture(scope="module")
def reg_fp32(tmp_path_factory):
    return device_listing(tmp_path_factory, "step_d3q19_reg")


def slot(name):
    """(VEC, COLL, HASBC, FLAGS) of a mangled k_step<D3Q19, float, float, ...>"""
    return tuple(int(v) for v in re.search(r"5D3Q19EffLi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name).groups())


def test_fp32_kernels_of_the_d3q19_unit_use_no_scratch(reg_fp32):
    """Every FP32FP32 instantiation of k_step in the unit must have .private_segment_fixed_size: 0 (4 collisions x VEC 1 / 2 / 4 x
    HASBC 0 / 1 / 2 x 2 load flags = 72 kernels).  With the compiler's defaults 12 of them reserve one, all in the extended-boundary
    variant (HASBC = 2): f[4][q] in scratch at VEC = 4 because the loop over a thread's cells is not unrolled (320 B), and a dead 36 B
    slot in the forced VEC = 1 kernels; the unit's two flags in the Makefile remove both (profiles/regularized_collision.md)."""
    assert len(reg_fp32) == 72, len(reg_fp32)
    for name, size, vgprs in reg_fp32:
        print(f"{slot(name)}: private segment {size} B, {vgprs} VGPRs")
    spilled = [(slot(name), size) for name, size, _ in reg_fp32 if size != 0]
    assert not spilled, spilled
