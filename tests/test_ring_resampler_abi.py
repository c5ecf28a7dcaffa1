"""CPU tests (no GPU) of the ring resampler's C ABI (gc_ring_resampler_*, gc_resampler_design): the declarations compile as C and
C++, the configuration is checked before anything needs a device, and the designed bank is the polyphase split of the library's own
low-pass, exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_ring_resampler_create", "gc_ring_resampler_destroy", "gc_ring_resampler_update", "gc_ring_resampler_info", "gc_resampler_design",
    "gc_resampler_conf_size"]


def test_header_with_ring_resampler_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_create)(gc_ctx*, gc_stream*, const gc_resampler_conf*, gc_stream*, gc_ring_resampler**) = gc_ring_resampler_create;\n'
            'static gc_status (*const f_destroy)(gc_ring_resampler*) = gc_ring_resampler_destroy;\n'
            'static gc_status (*const f_update)(gc_ring_resampler*, uint64_t*, uint64_t*) = gc_ring_resampler_update;\n'
            'static gc_status (*const f_info)(gc_ring_resampler*, uint64_t*, uint64_t*) = gc_ring_resampler_info;\n'
            'static gc_status (*const f_design)(double, double, uint32_t, float*, int, int*) = gc_resampler_design;\n'
            'int main(void){ gc_resampler_conf c; c.mode = GC_RESAMP_POLYPHASE; (void)c; (void)f_create; (void)f_destroy; (void)f_update; (void)f_info;\n'
            ' (void)f_design; return sizeof(gc_resampler_conf) == 40 && GC_RESAMP_DIRECT == 0 ? 0 : 1; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        exe = str(tmp_path / (name + ".exe"))
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", exe + ".o"])


def test_library_exports_the_ring_resampler_symbols():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert lib.gc_resampler_conf_size() == C.sizeof(gnsscorr.ResamplerConf) == 40
    assert hasattr(gnsscorr, "RingResampler") and hasattr(gnsscorr, "resampler_design")
    assert (gnsscorr.GC_RESAMP_DIRECT, gnsscorr.GC_RESAMP_POLYPHASE) == (0, 1)


def _create(conf):
    import gnsscorr
    lib = gnsscorr.load_library()
    out = C.c_void_p()
    st = lib.gc_ring_resampler_create(None, None, C.byref(conf) if conf is not None else None, None, C.byref(out))
    assert not out.value
    return st, lib.gc_last_error().decode()


def _conf(mode, fs_in, fs_out, phases=0, taps=0, bank=None):
    import gnsscorr
    return gnsscorr.ResamplerConf(fs_in, fs_out, mode, phases, taps, 0, None if bank is None else bank.ctypes.data_as(C.POINTER(C.c_float)))


BANK = np.ones(8192 + 1024, np.float32)


@pytest.mark.parametrize("mode, fs_in, fs_out, phases, taps, with_bank, word", [
    (2, 4e6, 1e6, 0, 0, False, "unknown mode"), (-1, 4e6, 1e6, 0, 0, False, "unknown mode"),
    (0, 0.0, 1e6, 0, 0, False, "finite and positive"), (0, 4e6, -1.0, 0, 0, False, "finite and positive"),
    (0, float("nan"), 1e6, 0, 0, False, "finite and positive"), (1, 4e6, float("inf"), 4, 4, True, "finite and positive"),
    (0, 65e6, 1e6, 0, 0, False, "outside 1/64 .. 64"), (0, 1e6, 64.5e6, 0, 0, False, "outside 1/64 .. 64"),
    (1, 65e6, 1e6, 4, 4, True, "outside 1/8 .. 64"), (1, 1e6, 8.5e6, 4, 4, True, "outside 1/8 .. 64"),
    (1, 25e6, 10e6, 0, 4, True, "0 phases"), (1, 25e6, 10e6, 3, 4, True, "3 phases"), (1, 25e6, 10e6, 512, 4, True, "512 phases"),
    (1, 25e6, 10e6, 4, 0, True, "0 taps per phase"), (1, 25e6, 10e6, 4, 1025, True, "1025 taps per phase"),
    (1, 25e6, 10e6, 16, 1024, True, "a bank of 16 x 1024"), (1, 25e6, 10e6, 256, 33, True, "a bank of 256 x 33"),
    (1, 25e6, 10e6, 32, 61, False, "NULL bank"),
])
def test_configuration_is_checked_before_any_device_call(mode, fs_in, fs_out, phases, taps, with_bank, word):
    """No context exists on a machine without a GPU: every limit must be reported with NULL handles, with nothing created."""
    import gnsscorr
    st, msg = _create(_conf(mode, fs_in, fs_out, phases, taps, BANK if with_bank else None))
    assert st == gnsscorr.GC_ERR_INVALID and word in msg, msg


def test_null_configuration_bad_taps_and_null_handles():
    import gnsscorr
    lib = gnsscorr.load_library()
    st, msg = _create(None)
    assert st == gnsscorr.GC_ERR_INVALID and "NULL configuration" in msg
    bad = np.ones(8, np.float32)
    bad[5] = np.nan
    st, msg = _create(_conf(1, 25e6, 10e6, 2, 4, bad))
    assert st == gnsscorr.GC_ERR_INVALID and "tap 1 of phase 1 is not finite" in msg
    # configurations at the limits pass the checks and get as far as the handles
    for conf in (_conf(0, 64e6, 1e6), _conf(0, 1e6, 64e6), _conf(0, 4e6, 4e6), _conf(1, 64e6, 1e6, 8, 1024, BANK), _conf(1, 1e6, 8e6, 256, 32, BANK),
            _conf(1, 4e6, 4e6, 1, 1, BANK)):
        st, msg = _create(conf)
        assert st == gnsscorr.GC_ERR_INVALID and "NULL argument" in msg, msg
    assert lib.gc_ring_resampler_update(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_resampler_info(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_resampler_destroy(None) == gnsscorr.GC_OK


@pytest.mark.parametrize("fs_in, fs_out, P", [(25e6, 10e6, 32), (6.625e6, 4e6, 64), (4e6, 5e6, 16), (4e6, 4e6, 1), (16.368e6, 4.092e6, 8), (1e6, 8e6, 256)])
def test_designed_bank_is_the_polyphase_split_of_the_library_low_pass(fs_in, fs_out, P):
    import gnsscorr
    low = min(fs_in, fs_out)
    g = gnsscorr.fir_low_pass(float(P), P * fs_in, low / 2.1, low / 10.0)
    T = -(-len(g) // P)
    bank = gnsscorr.resampler_design(fs_in, fs_out, P)
    assert bank.dtype == np.float32 and bank.shape == (P, T)
    padded = np.concatenate([g, np.zeros(P * T - len(g), np.float32)])
    assert bank.tobytes() == np.ascontiguousarray(padded.reshape(T, P).T).tobytes()  # bank[p][k] == g[k P + p], zeros behind
    # every phase row passes DC with a gain near 1: the prototype's gain is P
    assert np.all(np.abs(bank.astype(np.float64).sum(axis=1) - 1.0) < 0.02)


def test_design_sizes_alone_limits_and_a_short_buffer():
    import gnsscorr
    lib = gnsscorr.load_library()
    fp = C.POINTER(C.c_float)
    t = C.c_int(-1)
    assert lib.gc_resampler_design(25e6, 10e6, 32, None, 0, C.byref(t)) == gnsscorr.GC_OK
    T = -(-len(gnsscorr.fir_low_pass(32.0, 32 * 25e6, 10e6 / 2.1, 1e6)) // 32)
    assert t.value == T
    assert lib.gc_resampler_design(25e6, 10e6, 32, None, 0, None) == gnsscorr.GC_OK
    buf = np.full(32 * T, 7.0, np.float32)
    assert lib.gc_resampler_design(25e6, 10e6, 32, buf.ctypes.data_as(fp), 32 * T - 1, C.byref(t)) == gnsscorr.GC_ERR_INVALID
    assert "do not fit" in lib.gc_last_error().decode() and np.all(buf == 7.0)
    assert lib.gc_resampler_design(25e6, 10e6, 32, buf.ctypes.data_as(fp), 32 * T, C.byref(t)) == gnsscorr.GC_OK and not np.any(buf == 7.0)
    # 64 -> 1 Msps: about 1542 taps per phase whatever P; 25 -> 10 Msps with 256 phases: 256 x 61 taps pass 8192
    for args in ((64e6, 1e6, 4), (64e6, 1e6, 1), (25e6, 10e6, 256)):
        t.value = -1
        assert lib.gc_resampler_design(args[0], args[1], args[2], None, 0, C.byref(t)) == gnsscorr.GC_ERR_INVALID, args
        assert "exceed" in lib.gc_last_error().decode() and t.value == 0
    for args in ((25e6, 10e6, 0), (25e6, 10e6, 12), (25e6, 10e6, 512), (0.0, 10e6, 4), (25e6, float("nan"), 4)):
        assert lib.gc_resampler_design(args[0], args[1], args[2], None, 0, C.byref(t)) == gnsscorr.GC_ERR_INVALID, args
