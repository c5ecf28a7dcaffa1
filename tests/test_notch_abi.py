"""CPU tests (no GPU) of the notch filter ring stage's C ABI (gc_ring_notch_*): the declarations compile as C and C++, the struct
has the stated size, the library exports the symbols, and every limit of the configuration is reported before anything needs a
device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_notch_conf_size", "gc_ring_notch_create", "gc_ring_notch_destroy", "gc_ring_notch_update", "gc_ring_notch_info", "gc_ring_notch_state"]


def test_header_with_ring_notch_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_create)(gc_ctx*, gc_stream*, const gc_notch_conf*, gc_stream*, gc_ring_notch**) = gc_ring_notch_create;\n'
            'static gc_status (*const f_destroy)(gc_ring_notch*) = gc_ring_notch_destroy;\n'
            'static gc_status (*const f_update)(gc_ring_notch*, uint64_t*, uint64_t*) = gc_ring_notch_update;\n'
            'static gc_status (*const f_info)(gc_ring_notch*, uint64_t*, uint64_t*) = gc_ring_notch_info;\n'
            'static gc_status (*const f_state)(gc_ring_notch*, uint64_t*, uint64_t*, float*, uint32_t*, int32_t*, float*, float*) = gc_ring_notch_state;\n'
            'int main(void){ gc_notch_conf c; c.mode = GC_NOTCH_LITE; c.noise_floor = GC_NOTCH_FLOOR_LINEAR; (void)c; (void)f_create; (void)f_destroy;\n'
            ' (void)f_update; (void)f_info; (void)f_state; return 0; }\n'
            'typedef char conf_is_48_bytes[sizeof(gc_notch_conf) == 48 && GC_NOTCH_FULL == 0 && GC_NOTCH_FLOOR_REFERENCE == 0 ? 1 : -1];\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / (name + ".o"))])


def test_library_exports_the_ring_notch_symbols():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert lib.gc_notch_conf_size() == C.sizeof(gnsscorr.NotchConf) == 48
    assert hasattr(gnsscorr, "RingNotch") and hasattr(gnsscorr.RingNotch, "state")
    assert (gnsscorr.GC_NOTCH_FULL, gnsscorr.GC_NOTCH_LITE, gnsscorr.GC_NOTCH_FLOOR_REFERENCE, gnsscorr.GC_NOTCH_FLOOR_LINEAR) == (0, 1, 0, 1)


def _conf(**kw):
    import gnsscorr
    v = dict(pfa=0.001, threshold=0.0, p_c_factor=0.9, length=32, segments_est=12500, segments_reset=5000000, segments_coeff=1, mode=0, noise_floor=0)
    v.update(kw)
    return gnsscorr.NotchConf(v["pfa"], v["threshold"], v["p_c_factor"], v["length"], v["segments_est"], v["segments_reset"], v["segments_coeff"], v["mode"],
        v["noise_floor"])


def _create(conf):
    import gnsscorr
    lib = gnsscorr.load_library()
    out = C.c_void_p()
    st = lib.gc_ring_notch_create(None, None, C.byref(conf) if conf is not None else None, None, C.byref(out))
    assert not out.value
    return st, lib.gc_last_error().decode()


@pytest.mark.parametrize("kw, word", [
    (dict(mode=2), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(noise_floor=2), "unknown noise floor"),
    (dict(length=1), "length 1 is outside"), (dict(length=0), "length 0 is outside"), (dict(length=1025), "length 1025 is outside"),
    (dict(p_c_factor=1.0), "p_c_factor"), (dict(p_c_factor=-0.1), "p_c_factor"), (dict(p_c_factor=float("nan")), "p_c_factor"),
    (dict(pfa=0.0), "pfa"), (dict(pfa=1.0), "pfa"), (dict(pfa=float("nan")), "pfa"),
    (dict(threshold=-1.0), "threshold"), (dict(threshold=float("inf")), "threshold"),
    (dict(segments_est=0), "segments_est"), (dict(segments_coeff=0), "segments_coeff"),
])
def test_configuration_is_checked_before_any_device_call(kw, word):
    """No context exists on a machine without a GPU: every limit must be reported with NULL handles, with nothing created."""
    import gnsscorr
    st, msg = _create(_conf(**kw))
    assert st == gnsscorr.GC_ERR_INVALID and word in msg, msg


def test_null_configuration_limits_and_null_handles():
    import gnsscorr
    lib = gnsscorr.load_library()
    st, msg = _create(None)
    assert st == gnsscorr.GC_ERR_INVALID and "NULL configuration" in msg
    # configurations at the limits pass the checks and get as far as the handles
    for kw in (dict(length=2), dict(length=1024), dict(p_c_factor=0.0), dict(p_c_factor=0.999), dict(segments_est=1, segments_reset=0), dict(mode=1, segments_coeff=7),
            dict(noise_floor=1, threshold=1000.0), dict(pfa=0.5)):
        st, msg = _create(_conf(**kw))
        assert st == gnsscorr.GC_ERR_INVALID and "NULL argument" in msg, msg
    assert lib.gc_ring_notch_update(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_notch_info(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_notch_state(None, None, None, None, None, None, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_ring_notch_destroy(None) == gnsscorr.GC_OK
