"""GPU test of the two-hypothesis Galileo E1 adapters of the C++ drop-in layer (gnss-sdr-1_amd/adapter/): the CCCWSR and 8 ms
AcquisitionInterface adapters over hip_pcps_paired_acquisition and hip_acquisition_bank's CCCWSR option, on the Galileo E1 capture
of tests/golden (paired_acquisition_selftest.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_paired_acquisition_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "paired_acquisition_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "paired_acquisition_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "paired acquisition self-test passed" in p.stdout
