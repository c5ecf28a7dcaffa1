"""GPU test of the fine Doppler pieces of the C++ drop-in layer (fine_doppler_selftest.cpp), on synthetic GPS L1 C/A at 4 Msps:
  - GpsL1CaPcpsAcquisitionFineDopplerHip over hip_pcps_acquisition_fine_doppler, the image of pcps_acquisition_fine_doppler_cc: a
    satellite at -1762.5 Hz searched with a 500 Hz step and two dwells is declared, its Doppler reported within one fine bin
    (12.5 Hz), with the block's stamps and sample counts; a noise-only search ends negative;
  - hip_acquisition_bank with fine_doppler = true: the three satellites present among five PRNs are refined to within one fine bin in
    one call, the other two are absent; the same search with the flag off is bit-identical to the bank built without the parameter;
    a ring that does not hold the ten code periods leaves the coarse values and reports why."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_fine_doppler_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "fine_doppler_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "fine_doppler_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "fine doppler self-test passed" in p.stdout
    assert "fine -1762.5 Hz" in p.stdout
    assert p.stdout.count("bank: PRN") == 3
