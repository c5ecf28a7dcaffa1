"""CPU tests (no GPU) of the ring decimator's C ABI (gc_ring_decimator_*, gc_acq_resampler_plan): the declarations compile as C and
C++, the library exports them, the arguments are checked before anything needs a device, and the acquisition resampler's plan is
the reference's rule (src/core/receiver/gnss_flowgraph.cc:430-452) plus this library's limits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_ring_decimator_create", "gc_ring_decimator_destroy", "gc_ring_decimator_update", "gc_ring_decimator_info", "gc_acq_resampler_plan"]
# (fs_in, opt) -> (decimation, taps): the reference's rule and the formula in gnsscorr.h
PLANS = [
    (4_000_000, 1_000_000, 4, 97), (5_000_000, 1_000_000, 5, 121), (6_625_000, 1_000_000, 5, 121), (2_600_000, 1_000_000, 2, 49),
    (12_500_000, 1_000_000, 10, 241), (16_368_000, 1_000_000, 16, 385), (25_000_000, 1_000_000, 25, 603), (25_000_000, 2_000_000, 10, 241),
    (25_000_000, 10_000_000, 2, 49),
]


def test_header_with_ring_decimator_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_create)(gc_ctx*, gc_stream*, uint32_t, const float*, uint32_t, gc_stream*, gc_ring_decimator**) = gc_ring_decimator_create;\n'
            'static gc_status (*const f_destroy)(gc_ring_decimator*) = gc_ring_decimator_destroy;\n'
            'static gc_status (*const f_update)(gc_ring_decimator*, uint64_t*, uint64_t*) = gc_ring_decimator_update;\n'
            'static gc_status (*const f_info)(gc_ring_decimator*, uint64_t*, uint64_t*) = gc_ring_decimator_info;\n'
            'static gc_status (*const f_plan)(int64_t, uint32_t, uint32_t*, int64_t*, float*, int, int*, uint32_t*) = gc_acq_resampler_plan;\n'
            'int main(void){ (void)f_create; (void)f_destroy; (void)f_update; (void)f_info; (void)f_plan; return 0; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])


def test_library_exports_the_ring_decimator_symbols_and_the_abi_check_is_green():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert lib.gc_abi_check(C.sizeof(gnsscorr.EpochParams), C.sizeof(gnsscorr.LoopConf), gnsscorr.LOOP_RECORD_DTYPE.itemsize, C.sizeof(gnsscorr.LoopSyncConf),
        C.sizeof(gnsscorr.AcqConf), C.sizeof(gnsscorr.AcqResult)) == gnsscorr.GC_OK
    assert hasattr(gnsscorr, "RingDecimator") and hasattr(gnsscorr, "acq_resampler_plan")


@pytest.mark.parametrize("fs, opt, D, T", PLANS)
def test_plan_is_the_reference_rule(fs, opt, D, T):
    import gnsscorr
    d, rfs, taps, latency = gnsscorr.acq_resampler_plan(fs, opt)
    assert (d, len(taps)) == (D, T) and rfs == fs // D and fs % D == 0
    assert latency == (T - 1) // 2
    ref = gnsscorr.fir_low_pass(1.0, fs, rfs / 2.1, rfs / 10)
    assert taps.dtype == np.float32 and taps.tobytes() == ref.tobytes()


@pytest.mark.parametrize("fs", [1_000_000, 1_500_000])
def test_plan_is_disabled_when_the_input_rate_is_too_low(fs):
    import gnsscorr
    d, rfs, taps, latency = gnsscorr.acq_resampler_plan(fs, 1_000_000)
    assert (d, rfs, len(taps), latency) == (1, fs, 0, 0)


def test_plan_keeps_within_the_kernel_limits():
    """100 Msps with a 1 Msps optimum: the reference's rule alone gives D = 100 (and about 2409 taps); the library goes on to the next
    divisor whose filter fits."""
    import gnsscorr
    fs = 100_000_000
    d, rfs, taps, latency = gnsscorr.acq_resampler_plan(fs, 1_000_000)
    assert 1 < d <= 64 and 1 <= len(taps) <= 1024 and fs % d == 0 and rfs == fs // d and latency == (len(taps) - 1) // 2
    assert taps.tobytes() == gnsscorr.fir_low_pass(1.0, fs, rfs / 2.1, rfs / 10).tobytes()
    # the next divisor below: no divisor of fs between d and 64 has a filter of at most 1024 taps
    for bigger in range(d + 1, 65):
        if fs % bigger == 0:
            assert len(gnsscorr.fir_low_pass(1.0, fs, fs / bigger / 2.1, fs / bigger / 10)) > 1024


def test_plan_sizes_alone_and_a_short_buffer():
    import gnsscorr
    lib = gnsscorr.load_library()
    d, rfs, n, lat = C.c_uint32(0), C.c_int64(0), C.c_int(0), C.c_uint32(0)
    assert lib.gc_acq_resampler_plan(25_000_000, 1_000_000, C.byref(d), C.byref(rfs), None, 0, C.byref(n), C.byref(lat)) == gnsscorr.GC_OK
    assert (d.value, rfs.value, n.value, lat.value) == (25, 1_000_000, 603, 301)
    buf = np.zeros(10, np.float32)
    assert lib.gc_acq_resampler_plan(25_000_000, 1_000_000, C.byref(d), C.byref(rfs), buf.ctypes.data_as(C.POINTER(C.c_float)), 10, C.byref(n),
        C.byref(lat)) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_resampler_plan(25_000_000, 1_000_000, None, None, None, 0, None, None) == gnsscorr.GC_OK
    assert lib.gc_acq_resampler_plan(0, 1_000_000, None, None, None, 0, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_resampler_plan(25_000_000, 0, None, None, None, 0, None, None) == gnsscorr.GC_ERR_INVALID


@pytest.mark.parametrize("decimation, n_taps, null_taps, word", [
    (0, 8, False, "decimation"), (65, 8, False, "decimation"), (4, 0, False, "taps"), (4, 1025, False, "taps"), (4, 8, True, "taps")])
def test_arguments_are_checked_before_any_device_call(decimation, n_taps, null_taps, word):
    """No context exists on a machine without a GPU: the limits must be reported with NULL handles, the same way everywhere."""
    import gnsscorr
    lib = gnsscorr.load_library()
    taps = np.zeros(1025, np.float32)
    out = C.c_void_p()
    tp = None if null_taps else taps.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.gc_ring_decimator_create(None, None, decimation, tp, n_taps, None, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert word in lib.gc_last_error().decode() and not out.value


def test_null_handles_are_refused_without_gpu():
    import gnsscorr
    lib = gnsscorr.load_library()
    one = np.ones(1, np.float32)
    out = C.c_void_p()
    assert lib.gc_ring_decimator_create(None, None, 1, one.ctypes.data_as(C.POINTER(C.c_float)), 1, None, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert "NULL argument" in lib.gc_last_error().decode()
    bad = np.array([np.nan], np.float32)
    assert lib.gc_ring_decimator_create(None, None, 1, bad.ctypes.data_as(C.POINTER(C.c_float)), 1, None, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_decimator_update(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_decimator_info(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_decimator_destroy(None) == gnsscorr.GC_OK


@pytest.mark.parametrize("n_fft", [1000, 10000, 12500])
def test_acquisition_transform_plan_accepts_the_sizes_of_the_plans(n_fft):
    """GPS L1 at 1 Msps (N = 1000), Galileo E1 at 2.5 Msps (4 ms: N = 10000), L5 / E5a at 12.5 Msps (N = 12500).  gc_acq_create needs
    a context before it gets to the transform plan, so the host-side plan maker the engine calls (acq_plan_make, csrc/acq_kernels.h,
    with gc_acq_create's LDS limit) is called directly: it must factor every size into N1 x N2 with N1 x N2 = N."""
    import gnsscorr
    lib = gnsscorr.load_library()
    make = getattr(lib, "_Z13acq_plan_makeP10AcqFftPlanim")  # bool acq_plan_make(AcqFftPlan*, int, size_t)
    make.restype = C.c_bool
    make.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    plan = (C.c_int * 1024)()  # AcqFftPlan begins with N, N1, N2 and is far smaller than this
    assert make(C.cast(plan, C.c_void_p), n_fft, 160 * 1024), "no transform plan for N = %d" % n_fft
    assert plan[0] == n_fft and plan[1] >= 1 and plan[1] * plan[2] == n_fft, list(plan[:3])
    assert not make(C.cast(plan, C.c_void_p), 0, 160 * 1024)
