"""CPU: the device planner harness of tests/test_gpu_otg_planner.py (tests/cpp/otg_planner_device.hip) still
cross-compiles for gfx950 with the flags of sai2b_otg_n*.o, for both the 7- and the 8-joint build, so that a change to
the planner headers that breaks it fails without a GPU too."""
import os
import shutil
import subprocess

import pytest

import otg_planner_rows as op


@pytest.mark.skipif(not os.path.exists(op.HIPCC) and shutil.which("hipcc") is None, reason="hipcc not found")
@pytest.mark.parametrize("n_joints", [7, 8])
def test_planner_harness_cross_compiles_for_gfx950(n_joints, tmp_path):
    out = str(tmp_path / "harness.o")
    subprocess.run([op.HIPCC, *op.hipcc_flags(n_joints), "--cuda-device-only", "-c", op.HARNESS, "-o", out], check=True, timeout=600)
    assert os.path.getsize(out) > 0
