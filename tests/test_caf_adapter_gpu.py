"""GPU test of the E5a CAF adapter of the C++ drop-in layer (gnss-sdr-1_amd/adapter/hip_e5a_noncoherent_iq_acquisition_caf.h):
GalileoE5aNoncoherentIQAcquisitionCafHip on synthetic E5a signals at 2 Msps (caf_selftest.cpp --gpu):
  - 3 ms, first code period sign-flipped, CAF over one bin to either side, the Pfa threshold: positive at delay 1234 with both
    components on hypothesis B; the Doppler is +500 Hz under EXACT arithmetic and the last bin under REFERENCE (the block's wrapped
    weights leave only the tail section positive);
  - a zero-padded search (one period + zeros, one hypothesis) and an absent PRN;
  - a two-dwell bit-transition search, from host items and from a ring: the first dwell's cell and stamp are kept."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_caf_selftest():
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "caf_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "caf_selftest"])
    # the C++ program links the HIP runtime itself (no torch in that process)
    p = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "caf self-test passed" in p.stdout
    for line in ("E5a CAF acquisition (exact): delay 1234 samples, Doppler 500 Hz", "E5a CAF acquisition (reference): delay 1234 samples, Doppler 1000 Hz",
            "E5a CAF acquisition, zero padded: delay 777 samples, Doppler -250 Hz"):
        assert line in p.stdout, line
