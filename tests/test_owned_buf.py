"""CPU test of the buffer owners of gnss-sdr-1_amd/csrc/gc_internal.h (gc_owned_buf with reserve, gc_mapped_buf): tests/owned_buf_selftest.cpp
runs them with a stub memory policy whose k-th call fails, for every k the create paths of the tracking host can reach, as a stand-alone
program under AddressSanitizer and UndefinedBehaviorSanitizer (a leak, a double free or a use after free ends it)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_include():
    """the HIP headers gc_internal.h names (declarations only: the stub policy calls nothing of the runtime)"""
    hipconfig = shutil.which("hipconfig")
    if hipconfig:
        return os.path.join(subprocess.check_output([hipconfig, "--path"], text=True).strip(), "include")
    return os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_owners_free_everything_once_whichever_call_fails(tmp_path):
    exe = str(tmp_path / "owned_buf_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
        "-I", hip_include(), "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "owned_buf_selftest.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
