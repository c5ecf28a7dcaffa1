"""CPU test of the scoped set of ring reads (gnss-sdr-1_amd/csrc/gc_read_set.h): a launch's reader slots are committed behind its
enqueue or cancelled on every other way out, each exactly once.  tests/read_set_selftest.cpp runs the exit paths against a fake
ring; also built with AddressSanitizer and UBSan when the toolchain has them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "read_set_selftest.cpp")
INCS = ["-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def _run(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, *INCS, SRC, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=60)


def test_every_ticket_is_released_exactly_once(tmp_path):
    p = _run(tmp_path, [], "rs")
    assert p.returncode == 0 and p.stdout.strip() == "0 failures", p.stdout + p.stderr


def test_every_ticket_is_released_exactly_once_under_asan_ubsan(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = subprocess.run(["g++", *san, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("AddressSanitizer / UBSan runtime not installed")
    p = _run(tmp_path, san, "rs_san")
    assert p.returncode == 0 and p.stdout.strip() == "0 failures" and "Sanitizer" not in p.stderr, p.stdout + p.stderr[-4000:]
