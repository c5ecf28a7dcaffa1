"""CPU test of the closed loop's launch plan (gnss-sdr-1_amd/csrc/trk_loop_plan.h): workgroup size and LDS code image of an engine,
printed by tests/loop_plan_selftest.cpp, against a table worked out by hand from the rules:

  header(threads) = threads / 64 * 16 floats: 256 / 128 / 64 floats = 1024 / 512 / 256 bytes at 1024 / 512 / 256 threads
  resident image  = (2 L + 64) floats, window = (L + 64) floats, both doubled for pilot tracking (the data replica)
  window instead of resident when 1024 + 4 * image > 150 KiB (153600), or > 64 KiB (65536) with more channels than CUs
  threads         = 1024 while 2 * channels <= CUs, 512 while channels <= 2 * CUs, else 256; forced; high-dynamics: always 256
  lds_bytes       = 4 * (header(threads) + image)
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# engine (see loop_plan_selftest.cpp) -> "threads lds_table_floats resident lds_bytes"
TABLE = [
    # GPS L1 C/A, data: image 2 * 1023 + 64 = 2110 floats, 1024 + 8440 = 9464 bytes: resident whatever the channel count
    ("32,256,0,0,0,1023,0", "1024 2110 1 9464"),  # 64 <= 256: 1024 threads
    ("128,256,0,0,0,1023,0", "1024 2110 1 9464"),  # 256 <= 256: still 1024
    ("129,256,0,0,0,1023,0", "512 2110 1 8952"),  # 258 > 256, 129 <= 512: 512 threads, 4 * (128 + 2110)
    ("512,256,0,0,0,1023,0", "512 2110 1 8952"),  # 512 <= 512: still 512; more channels than CUs, but 9464 <= 65536
    ("513,256,0,0,0,1023,0", "256 2110 1 8696"),  # 513 > 512: 256 threads, 4 * (64 + 2110)
    ("32,256,0,512,0,1023,0", "512 2110 1 8952"),  # forced 512 threads
    ("32,256,1,1024,0,1023,0", "256 2110 1 8696"),  # high-dynamics beats forced 1024: 256 threads and the 256-thread header
    # Galileo E1 pilot: (2 * 8184 + 64) * 2 = 32864 floats, 1024 + 131456 = 132480 bytes (131 KB) <= 153600
    ("32,256,0,0,0,8184,1", "1024 32864 1 132480"),
    # 257 channels on 256 CUs: 132480 > 65536: window (8184 + 64) * 2 = 16496; 514 > 256, 257 <= 512: 512 threads, 4 * (128 + 16496)
    ("257,256,0,0,0,8184,1", "512 16496 0 66496"),
    # 150 KiB: pilot, L = 9504: (19008 + 64) * 2 = 38144 floats, 1024 + 152576 = 153600, not above: resident
    ("32,256,0,0,0,9504,1", "1024 38144 1 153600"),
    # L = 9505: 38148 floats, 153616 > 153600: window (9505 + 64) * 2 = 19138, 4 * (256 + 19138)
    ("32,256,0,0,0,9505,1", "1024 19138 0 77576"),
    # 64 KiB with more channels than CUs: data, L = 8032: 16128 floats, 1024 + 64512 = 65536, not above: resident, 4 * (128 + 16128)
    ("257,256,0,0,0,8032,0", "512 16128 1 65024"),
    # L = 8033: 16130 floats, 65544 > 65536: window 8033 + 64 = 8097, 4 * (128 + 8097)
    ("257,256,0,0,0,8033,0", "512 8097 0 32900"),
    # the same length with a CU per channel (256 on 256) stays resident: 512 > 256, 256 <= 512: 512 threads, 4 * (128 + 16130)
    ("256,256,0,0,0,8033,0", "512 16130 1 65032"),
    # mixed: a 1023-sample data channel and a 10230-sample pilot, both started; the engine's own length and pilot mode do not count.
    # Resident need max(2110, (20460 + 64) * 2 = 41048): 1024 + 164192 = 165216 > 153600: window max(1087, (10230 + 64) * 2 = 20588)
    ("32,256,0,0,1,10230,0,1023/0/1,10230/1/1", "1024 20588 0 83376"),
    # mixed: the long slot is not started and does not count: the GPS image
    ("32,256,0,0,1,10230,0,1023/0/1,10230/1/0", "1024 2110 1 9464"),
    # n_cus = 0 means 256 CUs: the 128 / 129 channel rows again
    ("128,0,0,0,0,1023,0", "1024 2110 1 9464"),
    ("129,0,0,0,0,1023,0", "512 2110 1 8952"),
]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("loop_plan") / "loop_plan_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "loop_plan_selftest.cpp"), "-o", exe])
    return exe


def test_plan_equals_the_hand_worked_table(selftest):
    out = subprocess.run([selftest] + [engine for engine, _ in TABLE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(TABLE)
    for (engine, want), line in zip(TABLE, got):
        assert line == want, "engine %s: plan %s, expected %s" % (engine, line, want)
