"""CPU tests (no GPU) of the integer output rings' C ABI (gc_stream_accept_quantised_output, gc_conditioner_set_output_scale /
_output_info and the ring decimator's twins): the declarations compile as C and C++, the library exports them, the Python wrappers exist, every argument check that needs
no device is made before a handle is touched, and the host quantiser the GPU tests compare with does what the header states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conditioner_out_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_stream_accept_quantised_output", "gc_conditioner_set_output_scale", "gc_conditioner_output_info", "gc_ring_decimator_set_output_scale", "gc_ring_decimator_output_info"]


def test_header_with_output_formats_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_cs)(gc_conditioner*, float) = gc_conditioner_set_output_scale;\n'
            'static gc_status (*const f_ci)(gc_conditioner*, int32_t*, float*, uint64_t*) = gc_conditioner_output_info;\n'
            'static gc_status (*const f_ds)(gc_ring_decimator*, float) = gc_ring_decimator_set_output_scale;\n'
            'static gc_status (*const f_di)(gc_ring_decimator*, int32_t*, float*, uint64_t*) = gc_ring_decimator_output_info;\n'
            'static gc_status (*const f_acc)(gc_stream*) = gc_stream_accept_quantised_output;\n'
            'int main(void){ (void)f_acc; (void)f_cs; (void)f_ci; (void)f_ds; (void)f_di; return sizeof(gc_conditioner_conf) == 32 ? 0 : 1; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])


def test_library_exports_the_symbols_and_the_wrappers_exist():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert callable(getattr(gnsscorr.IqStream, "accept_quantised_output"))
    for cls in (gnsscorr.Conditioner, gnsscorr.RingDecimator):
        assert callable(getattr(cls, "set_output_scale")) and callable(getattr(cls, "output_info"))
    # the structures keep their sizes
    assert lib.gc_conditioner_conf_size() == C.sizeof(gnsscorr.ConditionerConf) == 32
    assert lib.gc_blanking_conf_size() == C.sizeof(gnsscorr.BlankingConf) == 24


@pytest.mark.parametrize("setter", ["gc_conditioner_set_output_scale", "gc_ring_decimator_set_output_scale"])
@pytest.mark.parametrize("scale", [0.0, -1.0, -0.0, float("inf"), float("-inf"), float("nan")])
def test_a_bad_scale_is_refused_before_the_handle_is_looked_at(setter, scale):
    """No context exists on a machine without a GPU: the scale is checked first, with a NULL handle, the same way everywhere."""
    import gnsscorr
    lib = gnsscorr.load_library()
    assert getattr(lib, setter)(None, scale) == gnsscorr.GC_ERR_INVALID
    msg = lib.gc_last_error().decode()
    assert setter in msg and "scale" in msg and "NULL" not in msg


def test_null_handles_are_refused_without_gpu():
    import gnsscorr
    lib = gnsscorr.load_library()
    fmt, scale, n = C.c_int32(-1), C.c_float(-1.0), C.c_uint64(77)
    assert lib.gc_stream_accept_quantised_output(None) == gnsscorr.GC_ERR_INVALID
    assert "gc_stream_accept_quantised_output: NULL handle" in lib.gc_last_error().decode()
    for setter, info in (("gc_conditioner_set_output_scale", "gc_conditioner_output_info"),
            ("gc_ring_decimator_set_output_scale", "gc_ring_decimator_output_info")):
        # a good scale gets as far as the handle
        assert getattr(lib, setter)(None, 127.0) == gnsscorr.GC_ERR_INVALID
        assert "NULL handle" in lib.gc_last_error().decode() and setter in lib.gc_last_error().decode()
        assert getattr(lib, info)(None, C.byref(fmt), C.byref(scale), C.byref(n)) == gnsscorr.GC_ERR_INVALID
        assert "NULL handle" in lib.gc_last_error().decode() and info in lib.gc_last_error().decode()
        assert getattr(lib, info)(None, None, None, None) == gnsscorr.GC_ERR_INVALID
    assert (fmt.value, scale.value, n.value) == (-1, -1.0, 77)  # nothing was written


def test_host_quantiser_follows_the_stated_order():
    """Clamp first, then round, ties to even; strict comparisons; NaN -> 0 and not clipped."""
    I16, I8 = conditioner_out_ref.GC_IQ_I16, conditioner_out_ref.GC_IQ_I8
    y = np.array([0.5 + 1.5j, 2.5 - 0.5j, -1.5 - 2.5j, 127.0 + 127.25j, 127.5 - 128.0j, -128.5 + 1e9j, complex(np.inf, -np.inf), complex(np.nan, 3.4)], np.complex64)
    q, clipped = conditioner_out_ref.quantise(y, I8)
    assert q.dtype == np.int8 and q.tolist() == [[0, 2], [2, 0], [-2, -2], [127, 127], [127, -128], [-128, 127], [127, -128], [0, 3]]
    assert clipped == 6  # 127.25, 127.5, -128.5, 1e9, +inf, -inf
    q, clipped = conditioner_out_ref.quantise(y, I16)
    assert q.dtype == np.int16 and q[5].tolist() == [-128, 32767] and q[6].tolist() == [32767, -32768] and clipped == 3
    # the product is float32: 1/3 * 3 rounds to 1 in float32
    q, clipped = conditioner_out_ref.quantise(np.array([np.float32(1.0) / np.float32(3.0) + 0j], np.complex64), I16, 3.0)
    assert q.tolist() == [[1, 0]] and clipped == 0
    q, clipped = conditioner_out_ref.quantise(np.array([0.5 + 1.0j, 1.5 - 1.01j], np.complex64), I8, 127.0)
    assert q.tolist() == [[64, 127], [127, -128]] and clipped == 2  # 63.5 -> 64 (even); 190.5 and -128.27 clip, 127.0 does not
