"""GPU test of the notch filter ring stage in the C++ drop-in layer: hip_notch_filter / hip_notch_filter_lite (the reference adapters'
keys plus noise_floor / threshold) behind a gr_complex ring at 4 Msps with a tone 30 dB above the noise -- hip_pcps_acquisition finds
the satellite on the notched ring and not on the raw samples (adapter/notch_selftest.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_notch_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "notch_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "notch_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "notch self-test passed" in p.stdout
