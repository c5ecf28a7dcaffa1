"""GPU test of the GLONASS device loop in the C++ drop-in layer (adapter/glonass_loop_selftest.cpp): the device-loop block
hip_glonass_ca_dll_pll_tracking_dev against the host-loop block hip_glonass_ca_dll_pll_tracking on the same samples, item by item
(the pull-in item included, Tracking_sample_counter equal, prompt / Doppler / C/N0 at the gates of tests/test_glonass_loop_gpu.py),
and hip_glonass_tracking_group with 4 slots of different frequency channels on one ring against 4 single blocks."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_glonass_loop_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "glonass_loop_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "glonass_loop_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "glonass_loop_selftest: ok" in p.stdout
