"""CPU test of the signal generator's closed forms (gnss-sdr-1_amd/csrc/siggen_phase.h): tests/siggen_phase_selftest.cpp, a
stand-alone program, compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_forms_against_increments_and_128_bit_integers(tmp_path):
    exe = str(tmp_path / "siggen_phase_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
        "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"), os.path.join(ROOT, "tests", "siggen_phase_selftest.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "siggen phase self-test passed" in p.stdout
