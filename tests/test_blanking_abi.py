"""CPU tests (no GPU) of the pulse-blanking C ABI (gc_conditioner_set_pulse_blanking, gc_conditioner_blanking_info,
gc_chi2_upper_quantile): the declarations compile as C and C++, the library exports them, the structure layout matches the binding,
the limits are checked before anything needs a device, the chi-squared quantile equals known values, and the 64-wide decision step
of the device kernel equals the sequential loop of the definition (tests/blank_decide_selftest.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blanking_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_blanking_conf_size", "gc_conditioner_set_pulse_blanking", "gc_conditioner_blanking_info", "gc_chi2_upper_quantile"]
# scipy 1.15 chi2.isf(pfa, dof)
QUANTILES = [(64, 0.04, 85.11328962683008), (64, 0.001, 104.71632526304059), (16, 0.04, 27.1356342618495), (500, 0.01, 576.4928125116545),
    (2048, 0.001, 2251.487467571173), (2, 0.5, 1.386294361119891), (8192, 1e-6, 8814.898355762509)]


def test_header_with_blanking_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_set)(gc_conditioner*, const gc_blanking_conf*) = gc_conditioner_set_pulse_blanking;\n'
            'static gc_status (*const f_info)(gc_conditioner*, uint64_t*, uint64_t*, float*, uint32_t*, float*) = gc_conditioner_blanking_info;\n'
            'static gc_status (*const f_q)(double, double, double*) = gc_chi2_upper_quantile;\n'
            'static size_t (*const f_size)(void) = gc_blanking_conf_size;\n'
            'int main(void){ gc_blanking_conf b; gc_conditioner_conf c; b.pfa = 0.04f; b.threshold = 0.0f; b.length = 32; b.segments_est = 12500;\n'
            '  b.segments_reset = 5000000; b.reserved = 0; (void)f_set; (void)f_info; (void)f_q; (void)f_size; (void)c;\n'
            '  return (sizeof b == 24 && sizeof c == 32 && b.length == 32) ? 0 : 1; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        exe = str(tmp_path / (name + ".exe"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-c", "-o", exe + ".o"])


def test_library_exports_the_blanking_symbols():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name


def test_blanking_conf_layout_matches_the_binding():
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_blanking_conf_size() == C.sizeof(gnsscorr.BlankingConf) == 24
    assert lib.gc_conditioner_conf_size() == 32  # untouched
    B = gnsscorr.BlankingConf
    assert (B.pfa.offset, B.threshold.offset, B.length.offset, B.segments_est.offset, B.segments_reset.offset) == (0, 4, 8, 12, 16)


@pytest.mark.parametrize("change, word", [
    (dict(length=0), "length"), (dict(length=4097), "length"),
    (dict(pfa=0.0), "pfa"), (dict(pfa=1.0), "pfa"), (dict(pfa=-0.1), "pfa"), (dict(pfa=float("nan")), "pfa"),
    (dict(segments_est=0), "segments_est"),
    (dict(threshold=-1.0), "threshold"), (dict(threshold=float("inf")), "threshold"), (dict(threshold=float("nan")), "threshold"),
])
def test_blanking_limits_are_checked_before_any_device_call(change, word):
    """No conditioner exists on a machine without a GPU: the limits must be reported with a NULL handle, the same way everywhere."""
    import gnsscorr
    lib = gnsscorr.load_library()
    fields = dict(pfa=0.04, threshold=0.0, length=32, segments_est=12500, segments_reset=5000000, reserved=0)
    fields.update(change)
    conf = gnsscorr.BlankingConf(**fields)
    assert lib.gc_conditioner_set_pulse_blanking(None, C.byref(conf)) == gnsscorr.GC_ERR_INVALID
    assert word in lib.gc_last_error().decode()


def test_null_handles_are_refused_without_gpu():
    import gnsscorr
    lib = gnsscorr.load_library()
    for fields in (dict(pfa=0.04, threshold=0.0, length=32, segments_est=12500, segments_reset=5000000, reserved=0),
            dict(pfa=0.5, threshold=3.5, length=4096, segments_est=1, segments_reset=0, reserved=0),
            dict(pfa=0.001, threshold=0.0, length=1, segments_est=1, segments_reset=0xffffffff, reserved=0)):
        conf = gnsscorr.BlankingConf(**fields)  # valid: gets as far as the handle
        assert lib.gc_conditioner_set_pulse_blanking(None, C.byref(conf)) == gnsscorr.GC_ERR_INVALID
        assert "NULL handle" in lib.gc_last_error().decode()
    assert lib.gc_conditioner_set_pulse_blanking(None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_conditioner_blanking_info(None, None, None, None, None, None) == gnsscorr.GC_ERR_INVALID
    assert "NULL handle" in lib.gc_last_error().decode()


@pytest.mark.parametrize("dof, pfa, literal", QUANTILES)
def test_chi2_upper_quantile_matches_known_values(dof, pfa, literal):
    import gnsscorr
    got = gnsscorr.chi2_upper_quantile(dof, pfa)
    print("chi2 upper quantile dof=%g pfa=%g: %.16g, literal %.16g, relative difference %.2e" % (dof, pfa, got, literal, abs(got - literal) / literal))
    assert abs(got - literal) <= 1e-9 * literal


@pytest.mark.parametrize("dof, pfa", [(64, 0.0), (64, 1.0), (64, -0.5), (64, 1.5), (64, float("nan")), (0, 0.04), (-2, 0.04), (float("nan"), 0.04)])
def test_chi2_upper_quantile_refuses_bad_arguments(dof, pfa):
    import gnsscorr
    lib = gnsscorr.load_library()
    out = C.c_double(-1.0)
    assert lib.gc_chi2_upper_quantile(float(dof), float(pfa), C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_chi2_upper_quantile(64.0, 0.04, None) == gnsscorr.GC_ERR_INVALID


def test_decision_step_equals_the_sequential_loop(tmp_path):
    exe = str(tmp_path / "blank_decide_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "blank_decide_selftest.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "agrees with the sequential loop bit for bit" in p.stdout


def test_restatement_follows_the_definition():
    """The float64 restatement itself on a hand-checked stream: L = 2, two estimation segments, a pulse, a reset with the quirk
    (n becomes 1: the new estimate is the mean of the old floor and ONE new segment), and a partial segment left undecided."""
    x = np.array([1, 1, 1, 1, 10, 10, 1, 1, 2, 2, 1, 1, 9], np.float64).astype(np.complex64)
    r = blanking_ref.blank(x, 2, threshold=3.0, segments_est=2, segments_reset=2)
    # E = 2 2 200 2 8 2; noise after two segments = 0.5; s2: 400 > 3 blank (n 3); s3: 4 > 3 blank (n 4); s4 (E 8): 16 > 3 blank ... so
    # every later segment is blanked with this floor: check exactly that, then a run with a higher threshold for the reset
    assert r["flags"].tolist() == [False, False, True, True, True, True] and r["decided"] == 6 and r["noise"] == 0.5 and r["n"] == 6
    r = blanking_ref.blank(x, 2, threshold=20.0, segments_est=2, segments_reset=2)
    # s2: 400 blank (n 3); s3: 4 pass, n = 3 > 2: reset, n = 1; s4: estimate, noise = (1 * 0.5 + 8 / 4) / 2 = 1.25, n = 2; s5: 1.6 pass
    assert r["flags"].tolist() == [False, False, True, False, False, False] and r["noise"] == 1.25 and r["n"] == 3 and r["resets"] == 1
    assert np.isnan(r["ratio"][[0, 1, 4]]).all() and r["ratio"][2] == 20.0 and r["last_filtered"] is False
    y = blanking_ref.apply(x, 2, r["flags"])
    assert np.array_equal(y[4:6], [0, 0]) and np.array_equal(np.delete(y, [4, 5]), np.delete(x, [4, 5]))
    assert blanking_ref.margin(32, 40) == (32 + 40 + 16) * 2.0 ** -23
