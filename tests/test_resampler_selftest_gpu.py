"""GPU test of the ring resampler in the C++ drop-in layer: hip_direct_resampler (the reference's Direct_Resampler keys plus
resampler_mode / phases) behind a cshort ring at 6.625 Msps -- direct mode's picks, and hip_pcps_acquisition at N = 4000 on the ring
derived polyphase to 4 Msps (adapter/resampler_selftest.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_resampler_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "resampler_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "resampler_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "resampler self-test passed" in p.stdout
