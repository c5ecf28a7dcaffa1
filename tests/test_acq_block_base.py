"""CPU test (no GPU) of what the acquisition block images of the C++ drop-in layer share (adapter/acquisition_block_base.h,
adapter/acquisition_adapter_base.h) through adapter/acq_block_selftest.cpp: the item blocks' state machine driven by scripted blocks
for each of the four state numberings and policies, the inclusive Doppler-bin count, the Pfa -> threshold rule bit for bit against
the rule it replaced, and every real block's init() and error path without a device -- built through the Makefile, and once more as a
stand-alone program under ASan / UBSan.  `paired_acquisition_selftest --host` checks what a Doppler step of 0 does in the paired
block and in the 8 ms adapter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter")
# the program checks the blocks' "no device" paths: it sees none, wherever it runs
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


def test_acq_block_selftest():
    subprocess.check_call(["make", "-s", "-C", ADAPTER, "acq_block_selftest"])
    p = subprocess.run([os.path.join(ADAPTER, "acq_block_selftest")], capture_output=True, text=True, timeout=60, env=dict(os.environ, **NO_DEVICE))
    assert p.returncode == 0 and "acq block self-test passed" in p.stdout, p.stdout + p.stderr


def test_acq_block_selftest_under_asan_ubsan(tmp_path):
    """The same stand-alone program (its own main, no GPU context) built with -fsanitize=address,undefined: the shared base, the real
    blocks' init() and conf filler and their error paths run clean."""
    exe = str(tmp_path / "acq_block_selftest_san")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
        "-I", os.path.join(ROOT, "include"), "-I", ADAPTER, os.path.join(ADAPTER, "acq_block_selftest.cpp"), "-o", exe,
        "-L", os.path.join(ROOT, "gnss-sdr-1_amd"), "-lgnsscorr", "-Wl,-rpath," + os.path.join(ROOT, "gnss-sdr-1_amd"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", **NO_DEVICE)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and "acq block self-test passed" in p.stdout, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]


def test_paired_host_side_pieces():
    """Bin count and the two step-0 refusals (block init() and the 8 ms adapter's Pfa rule), in a run that creates no GPU context."""
    subprocess.check_call(["make", "-s", "-C", ADAPTER, "paired_acquisition_selftest"])
    p = subprocess.run([os.path.join(ADAPTER, "paired_acquisition_selftest"), "--host"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "paired acquisition host self-test passed" in p.stdout, p.stdout + p.stderr
