"""CPU tests (no GPU) of the signal conditioner's C ABI (gc_conditioner_*, gc_stream_read, gc_fir_low_pass): the declarations
compile as C and C++, the library exports them, the structure layout matches the binding, the configuration is checked before
anything needs a device, and the low-pass design equals the formula the header states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conditioner_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_stream_read", "gc_conditioner_conf_size", "gc_conditioner_create", "gc_conditioner_destroy", "gc_conditioner_push",
    "gc_conditioner_push_pinned", "gc_conditioner_info", "gc_fir_low_pass"]


def test_header_with_conditioner_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_create)(gc_ctx*, const gc_conditioner_conf*, const float*, gc_stream*, gc_conditioner**) = gc_conditioner_create;\n'
            'static gc_status (*const f_push)(gc_conditioner*, const void*, uint64_t, uint64_t*, uint64_t*) = gc_conditioner_push;\n'
            'static gc_status (*const f_pin)(gc_conditioner*, const void*, uint64_t, uint64_t*, uint64_t*) = gc_conditioner_push_pinned;\n'
            'static gc_status (*const f_info)(gc_conditioner*, uint64_t*, uint64_t*) = gc_conditioner_info;\n'
            'static gc_status (*const f_destroy)(gc_conditioner*) = gc_conditioner_destroy;\n'
            'static gc_status (*const f_read)(gc_stream*, uint64_t, uint64_t, void*) = gc_stream_read;\n'
            'static gc_status (*const f_lp)(double, double, double, double, float*, int, int*) = gc_fir_low_pass;\n'
            'static size_t (*const f_size)(void) = gc_conditioner_conf_size;\n'
            'int main(void){ gc_conditioner_conf c; c.fs_in = 1.0; c.translate_hz = 0.0; c.decimation = 1; c.n_taps = 1; c.in_format = GC_IQ_I16; c.reserved = 0;\n'
            '  (void)f_create; (void)f_push; (void)f_pin; (void)f_info; (void)f_destroy; (void)f_read; (void)f_lp; (void)f_size;\n'
            '  return (sizeof c == 32 && c.n_taps == 1) ? 0 : 1; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])


def test_library_exports_the_conditioner_symbols():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name


def test_conf_layout_matches_the_binding():
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_conditioner_conf_size() == C.sizeof(gnsscorr.ConditionerConf) == 32
    assert gnsscorr.ConditionerConf.decimation.offset == 16 and gnsscorr.ConditionerConf.in_format.offset == 24


@pytest.mark.parametrize("change, word", [
    (dict(decimation=0), "decimation"), (dict(decimation=65), "decimation"),
    (dict(n_taps=0), "taps"), (dict(n_taps=1025), "taps"),
    (dict(translate_hz=8.1e6), "translate_hz"), (dict(translate_hz=-8.1e6), "translate_hz"),
    (dict(in_format=7), "format"), (dict(fs_in=0.0), "fs_in"),
])
def test_configuration_is_checked_before_any_device_call(change, word):
    """No context exists on a machine without a GPU: the limits must be reported with a NULL context, the same way everywhere."""
    import gnsscorr
    lib = gnsscorr.load_library()
    fields = dict(fs_in=16e6, translate_hz=1.25e6, decimation=4, n_taps=63, in_format=gnsscorr.GC_IQ_I16, reserved=0)
    fields.update(change)
    conf = gnsscorr.ConditionerConf(**fields)
    taps = np.zeros(1025, np.float32)
    out = C.c_void_p()
    assert lib.gc_conditioner_create(None, C.byref(conf), taps.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert word in lib.gc_last_error().decode() and not out.value


def test_null_arguments_are_refused_without_gpu():
    import gnsscorr
    lib = gnsscorr.load_library()
    conf = gnsscorr.ConditionerConf(16e6, 0.0, 1, 1, gnsscorr.GC_IQ_F32, 0)
    one = np.ones(1, np.float32)
    fp = C.POINTER(C.c_float)
    out = C.c_void_p()
    assert lib.gc_conditioner_create(None, C.byref(conf), None, None, C.byref(out)) == gnsscorr.GC_ERR_INVALID  # NULL taps
    assert "taps" in lib.gc_last_error().decode()
    assert lib.gc_conditioner_create(None, None, one.ctypes.data_as(fp), None, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    # a valid configuration gets as far as the handles
    assert lib.gc_conditioner_create(None, C.byref(conf), one.ctypes.data_as(fp), None, C.byref(out)) == gnsscorr.GC_ERR_INVALID
    assert "NULL argument" in lib.gc_last_error().decode()
    assert lib.gc_conditioner_push(None, None, 0, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_conditioner_push_pinned(None, None, 0, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_conditioner_info(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_conditioner_destroy(None) == gnsscorr.GC_OK
    assert lib.gc_stream_read(None, 0, 0, None) == gnsscorr.GC_ERR_INVALID


@pytest.mark.parametrize("gain, fs, cutoff, tw, n_expected", [
    (1.0, 16e6, 1.6e6, 612e3, 63), (1.0, 25e6, 2.0e6, 950e3, 63), (2.5, 4e6, 1.0e6, 300e3, 33), (1.0, 1.0, 0.25, 0.9, 3)])
def test_fir_low_pass_equals_the_stated_formula(gain, fs, cutoff, tw, n_expected):
    """Both sides evaluate the formula in float64 and round once to float32; the libms may differ in the last bit of a double,
    which can move that one rounding: each tap is within one float32 spacing of the numpy value, and sum(h) = gain."""
    import gnsscorr
    got = gnsscorr.fir_low_pass(gain, fs, cutoff, tw)
    ref = conditioner_ref.fir_low_pass(gain, fs, cutoff, tw)
    assert got.dtype == np.float32 and len(got) == len(ref) == n_expected and len(got) % 2 == 1
    assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32)))
    assert np.array_equal(got, got[::-1])
    assert abs(float(got.astype(np.float64).sum()) - gain) <= len(got) * 2.0 ** -24 * np.abs(ref).sum()


def test_fir_low_pass_reports_its_length_and_refuses_a_short_buffer():
    import gnsscorr
    lib = gnsscorr.load_library()
    n = C.c_int(0)
    assert lib.gc_fir_low_pass(1.0, 16e6, 1.6e6, 612e3, None, 0, C.byref(n)) == gnsscorr.GC_OK and n.value == 63
    buf = np.zeros(10, np.float32)
    assert lib.gc_fir_low_pass(1.0, 16e6, 1.6e6, 612e3, buf.ctypes.data_as(C.POINTER(C.c_float)), 10, C.byref(n)) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_fir_low_pass(1.0, 16e6, 9e6, 612e3, None, 0, C.byref(n)) == gnsscorr.GC_ERR_INVALID


def test_restatement_is_a_plain_copy_and_a_known_tone():
    """The float64 restatement itself: T = 1, D = 1, f = 0 copies; a tone at the translation frequency lands on DC with the
    filter's DC gain; the phase of sample n is a closed form of n (a block computed from an offset equals the slice)."""
    fs, f = 16e6, 1.25e6
    n = np.arange(4096)
    x = np.exp(2j * np.pi * f * n / fs).astype(np.complex64)
    assert np.array_equal(conditioner_ref.condition(x, [1.0], 1, 0.0, fs), x.astype(np.complex128))
    h = conditioner_ref.fir_low_pass(1.0, fs, 1.6e6, 612e3)
    y = conditioner_ref.condition(x, h, 4, f, fs)
    assert len(y) == 1024 and np.max(np.abs(y[32:] - 1.0)) < 1e-5  # float32 tone, 2^-32-turn phase steps
    assert np.allclose(conditioner_ref.mixer(1000, 50, f, fs), conditioner_ref.mixer(0, 1050, f, fs)[1000:], rtol=0, atol=0)
    assert np.array_equal(conditioner_ref.condition(x, h, 4, f, fs, first_out=100, n_out=50), y[100:150])
