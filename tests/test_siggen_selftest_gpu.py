"""GPU test of the signal generator in the C++ drop-in layer: hip_signal_generator (the reference's Signal_Generator keys) produces
configuration 1 of the reference's gps_l1_ca_pcps_acquisition_gsoc2013_test.cc into a ring, and hip_acquisition_bank on that ring and
the hip_pcps_acquisition block on its samples find the satellite within that test's limits (adapter/siggen_selftest.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_signal_generator_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "siggen_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "siggen_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "signal generator self-test passed" in p.stdout
