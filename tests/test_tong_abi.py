"""CPU tests (no GPU) of the Tong engine's C ABI (gc_acq_create_tong, gc_acq_tong_set_threshold, gc_acq_tong_status,
gc_acq_tong_search_stream, gc_tong_threshold): the symbols are declared, exported and bound, struct gc_acq_tong_status has the
binding's layout, the argument checks that need no device answer GC_ERR_INVALID, and the decision step shared by host and device
(csrc/acq_tong_decide.h) passes its hand-made sequences as a stand-alone program under ASan / UBSan."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gc_acq_create_tong", "gc_acq_tong_set_threshold", "gc_acq_tong_status", "gc_acq_tong_search_stream", "gc_tong_threshold")


def test_new_symbols_are_declared_exported_and_bound():
    import gnsscorr
    lib = gnsscorr.load_library()
    txt = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in gnsscorr.API, name
    assert callable(gnsscorr.tong_threshold)
    for m in ("set_threshold", "tong_search_stream", "tong_status"):
        assert hasattr(gnsscorr.PcpsAcquisition, m), m


def test_status_layout_and_header_compile_as_c_and_cpp(tmp_path):
    import gnsscorr
    S = gnsscorr.AcqTongStatus
    assert C.sizeof(S) == 12
    assert (S.state.offset, S.tong_count.offset, S.dwell_count.offset) == (0, 4, 8)
    assert (gnsscorr.TONG_RUNNING, gnsscorr.TONG_POSITIVE, gnsscorr.TONG_NEGATIVE) == (0, 1, 2)
    # the struct tag and the call share a name: the header must still be C and C++
    src = ('#include "gnsscorr.h"\n#include <stddef.h>\n'
        "typedef char a_[sizeof(struct gc_acq_tong_status) == 12 ? 1 : -1];\n"
        "typedef char b_[offsetof(struct gc_acq_tong_status, tong_count) == 4 && offsetof(struct gc_acq_tong_status, dwell_count) == 8 ? 1 : -1];\n"
        "typedef char c_[GC_ACQ_TONG_RUNNING == 0 && GC_ACQ_TONG_POSITIVE == 1 && GC_ACQ_TONG_NEGATIVE == 2 ? 1 : -1];\n"
        "int use(gc_acq* a, struct gc_acq_tong_status* s) { return (int)gc_acq_tong_status(a, s); }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++14")):
        f = tmp_path / name
        f.write_text(src)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(f), "-o", str(tmp_path / (name + ".o"))])


def test_argument_checks_need_no_device():
    import gnsscorr
    lib = gnsscorr.load_library()
    conf = gnsscorr.AcqConf(2000000, 1, 1, 2000.0, 2000.0, 2, 1000, 500, 1, 0, 1, 0, 0, 4, 125.0)
    h = C.c_void_p()
    assert lib.gc_acq_create_tong(None, C.byref(conf), 1, 1, 2, 3, C.byref(h)) == gnsscorr.GC_ERR_INVALID
    assert b"NULL" in lib.gc_last_error()
    assert lib.gc_acq_create_tong(None, None, 1, 1, 2, 3, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_tong_set_threshold(None, 1.0) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_tong_status(None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_tong_search_stream(None, None, 0, 1, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_tong_threshold(0.001, 4000, 5000, 250, None) == gnsscorr.GC_ERR_INVALID
    out = C.c_float()
    assert lib.gc_tong_threshold(0.001, 0, 5000, 250, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_tong_threshold(0.001, 4000, 5000, 0, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    # tong together with combine or folding_factor never reaches the library
    for kw in (dict(combine="max"), dict(folding_factor=2)):
        with pytest.raises(ValueError):
            gnsscorr.PcpsAcquisition(None, 1, 2000000, 1, 1, 2000.0, 2000.0, 2, 1000, 500, tong=(1, 2, 3), **kw)


def test_decision_step_under_asan_ubsan(tmp_path):
    """csrc/acq_tong_decide.h, the step acq_tong_decide_kernel runs per satellite, as a stand-alone program (its own main, no GPU)."""
    exe = str(tmp_path / "acq_tong_decide_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
        "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"), os.path.join(ROOT, "tests", "acq_tong_decide_selftest.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "all sequences as expected" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_host_side_pieces_of_the_adapter():
    """Bin count, keys and defaults, the threshold rule and the failure path of the C++ adapter, in a stand-alone program that creates
    no GPU context."""
    d = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter")
    subprocess.check_call(["make", "-s", "-C", d, "tong_selftest"])
    p = subprocess.run([os.path.join(d, "tong_selftest"), "--host"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "tong host self-test passed" in p.stdout, p.stdout + p.stderr
