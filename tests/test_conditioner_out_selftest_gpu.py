"""GPU test of the integer output rings in the C++ drop-in layer: hip_signal_conditioner with output_item_type "cshort" and "cbyte"
(and hip_ring_decimator with the same keys) against the host quantisation of the gr_complex run (adapter/conditioner_out_selftest.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_conditioner_out_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "conditioner_out_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "conditioner_out_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "conditioner output self-test passed" in p.stdout
