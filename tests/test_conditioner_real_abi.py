"""CPU tests (no GPU) of the conditioner's real raw formats (gc_raw_real_format: GC_RAW_REAL_F32 / _I16 / _I8 / _2BIT): the 2-bit
packing helpers, the configuration checks that need no device, and the header as C99.  That a gc_stream ring refuses the new
values needs a context (gc_stream_create looks at its context first): tests/test_conditioner_real_gpu.py holds that check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_2bit_layout_against_a_literal_table():
    """Sample 4b + i is bits 2i .. 2i + 1 of byte b, least-significant pair first, two's complement: 0 -> 00, 1 -> 01, -2 -> 10,
    -1 -> 11."""
    import gnsscorr
    table = [
        ([0, 0, 0, 0], 0x00), ([1, 0, 0, 0], 0x01), ([-2, 0, 0, 0], 0x02), ([-1, 0, 0, 0], 0x03),
        ([0, 1, 0, 0], 0x04), ([0, 0, 1, 0], 0x10), ([0, 0, 0, 1], 0x40), ([0, 0, 0, -2], 0x80), ([0, 0, 0, -1], 0xC0),
        ([1, -2, -1, 0], 0x39), ([-1, -1, -1, -1], 0xFF), ([-2, 1, -2, 1], 0x66), ([0, -1, 1, -2], 0x9C),
    ]
    for values, byte in table:
        got = gnsscorr.pack_2bit(np.array(values))
        assert got.dtype == np.uint8 and got.tolist() == [byte], (values, byte, got)
        assert gnsscorr.unpack_2bit(np.array([byte], np.uint8)).tolist() == values
        assert gnsscorr.unpack_2bit(np.array([byte], np.uint8).view(np.int8)).tolist() == values
    both = gnsscorr.pack_2bit(np.array([1, -2, -1, 0, 0, -1, 1, -2], np.int8))
    assert both.tolist() == [0x39, 0x9C]


def test_pack_2bit_round_trip_and_refusals():
    import gnsscorr
    v = np.random.Generator(np.random.PCG64(11)).integers(-2, 2, 4 * 1000).astype(np.int8)
    assert set(v.tolist()) == {-2, -1, 0, 1}
    packed = gnsscorr.pack_2bit(v)
    assert packed.shape == (1000,) and packed.dtype == np.uint8
    back = gnsscorr.unpack_2bit(packed)
    assert back.dtype == np.int8 and np.array_equal(back, v)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(gnsscorr.pack_2bit(gnsscorr.unpack_2bit(every)), every)
    assert gnsscorr.pack_2bit(np.zeros(0, np.int8)).shape == (0,) and gnsscorr.unpack_2bit(np.zeros(0, np.uint8)).shape == (0,)
    for bad in (np.zeros(6, np.int8), np.array([0, 0, 0, 2]), np.array([0, 0, 0, -3]), np.array([0.5, 0, 0, 0]), np.zeros((2, 4), np.int8)):
        with pytest.raises(ValueError):
            gnsscorr.pack_2bit(bad)


def test_constants():
    import gnsscorr
    assert (gnsscorr.GC_RAW_REAL_F32, gnsscorr.GC_RAW_REAL_I16, gnsscorr.GC_RAW_REAL_I8, gnsscorr.GC_RAW_REAL_2BIT) == (16, 17, 18, 19)
    assert (gnsscorr.GC_IQ_F32, gnsscorr.GC_IQ_I16, gnsscorr.GC_IQ_I8) == (0, 1, 2)


def _create(in_format):
    """gc_conditioner_create with a NULL context: the configuration is checked first, then the handles."""
    import gnsscorr
    lib = gnsscorr.load_library()
    conf = gnsscorr.ConditionerConf(16e6, 4e6, 4, 63, in_format, 0)
    taps = np.zeros(63, np.float32)
    out = C.c_void_p()
    st = lib.gc_conditioner_create(None, C.byref(conf), taps.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(out))
    assert not out.value
    return st, lib.gc_last_error().decode()


@pytest.mark.parametrize("in_format", [16, 17, 18, 19])
def test_the_real_formats_pass_the_configuration_check(in_format):
    """No device here: a valid configuration gets as far as the NULL handles, exactly as the complex formats do."""
    import gnsscorr
    st, msg = _create(in_format)
    assert st == gnsscorr.GC_ERR_INVALID and "NULL argument" in msg and "format" not in msg
    assert _create(gnsscorr.GC_IQ_I16)[1] == msg


@pytest.mark.parametrize("in_format", list(range(3, 16)) + [20, -1])
def test_values_between_the_two_enumerations_are_refused(in_format):
    import gnsscorr
    st, msg = _create(in_format)
    assert st == gnsscorr.GC_ERR_INVALID and "unknown input format %d" % in_format in msg


def test_push_and_blanking_refuse_null_handles_as_before():
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_conditioner_push(None, None, 6, None, None) == gnsscorr.GC_ERR_INVALID
    conf = gnsscorr.BlankingConf(0.04, 0.0, 32, 10, 100, 0)
    assert lib.gc_conditioner_set_pulse_blanking(None, C.byref(conf)) == gnsscorr.GC_ERR_INVALID
    assert "NULL handle" in lib.gc_last_error().decode()


def test_header_compiles_as_c99_with_the_real_formats(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'int main(void){ gc_conditioner_conf c; gc_raw_real_format f = GC_RAW_REAL_2BIT;\n'
            '  c.fs_in = 16e6; c.translate_hz = 4e6; c.decimation = 4; c.n_taps = 63; c.in_format = GC_RAW_REAL_I8; c.reserved = 0;\n'
            '  return (GC_RAW_REAL_F32 == 16 && GC_RAW_REAL_I16 == 17 && GC_RAW_REAL_I8 == 18 && (int)f == 19 && GC_IQ_I8 == 2 && sizeof c == 32\n'
            '      && c.in_format == 18) ? 0 : 1; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        exe = str(tmp_path / (name + ".exe"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
        assert subprocess.run([exe]).returncode == 0
