"""CPU tests (no GPU) of the ring's origin hook (gc_stream_debug_set_origin): the declaration compiles as C and C++, the library
exports the symbol, the Python wrapper has it, and a NULL handle is reported before anything needs a device.  What the hook does
to a ring needs one: tests/test_ring_origin_gpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_stream_debug_set_origin"]


def test_header_with_the_origin_hook_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_origin)(gc_stream*, uint64_t) = gc_stream_debug_set_origin;\n'
            'int main(void){ (void)f_origin; return 0; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / (name + ".o"))])


def test_library_exports_the_origin_hook():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert hasattr(gnsscorr.IqStream, "set_origin")


@pytest.mark.parametrize("origin", [0, 1, (1 << 40) + 12345, 1 << 62, (1 << 62) + 1, (1 << 64) - 1])
def test_null_handle_is_refused_without_a_device(origin):
    """The handle comes first: a NULL one is GC_ERR_INVALID whatever the origin, and the message names the function."""
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_stream_debug_set_origin(None, origin) == gnsscorr.GC_ERR_INVALID
    assert "gc_stream_debug_set_origin: NULL handle" in lib.gc_last_error().decode()
