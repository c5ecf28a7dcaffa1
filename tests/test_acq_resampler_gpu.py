"""GPU test of the acquisition resampler in the C++ drop-in layer: hip_acquisition_bank with use_acquisition_resampler (a derived
1 Msps ring made on the device by hip_ring_decimator) next to a bank without it, on one 4 Msps cshort ring, and the hand-over of
either bank's Gnss_Synchro to a hip_tracking_group on the full-rate ring (adapter/acq_resampler_selftest.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_acquisition_resampler_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "acq_resampler_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "acq_resampler_selftest"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "acquisition resampler self-test passed" in p.stdout
