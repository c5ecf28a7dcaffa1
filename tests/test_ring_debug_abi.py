"""CPU tests (no GPU) of the ring's two diagnostic calls (gc_stream_debug_read_storage, gc_stream_debug_guards): the declarations
compile as C and C++, the library exports the symbols, the Python wrapper has them, and NULL arguments are reported before
anything needs a device.  The range check needs a ring, so it is in tests/test_ring_contract_gpu.py."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gc_stream_debug_read_storage", "gc_stream_debug_guards"]


def test_header_with_the_diagnostic_calls_compiles_as_c_and_cpp(tmp_path):
    body = ('#include "gnsscorr.h"\n'
            'static gc_status (*const f_storage)(gc_stream*, uint64_t, uint64_t, void*) = gc_stream_debug_read_storage;\n'
            'static gc_status (*const f_guards)(gc_stream*, int32_t*, int32_t*) = gc_stream_debug_guards;\n'
            'int main(void){ (void)f_storage; (void)f_guards; return 0; }\n')
    for cc, std, name in (("gcc", "-std=c99", "t.c"), ("g++", "-std=c++11", "t.cpp")):
        src = tmp_path / name
        src.write_text(body)
        subprocess.check_call([cc, std, "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / (name + ".o"))])


def test_library_exports_the_diagnostic_calls():
    import gnsscorr
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API, name
    assert hasattr(gnsscorr.IqStream, "read_storage") and hasattr(gnsscorr.IqStream, "guards_intact")


def test_null_arguments_are_refused_without_a_device():
    import gnsscorr
    lib = gnsscorr.load_library()
    buf = (C.c_char * 16)()
    front, back = C.c_int32(7), C.c_int32(7)
    for n in (0, 1):
        assert lib.gc_stream_debug_read_storage(None, 0, n, buf) == gnsscorr.GC_ERR_INVALID
        assert "gc_stream_debug_read_storage: NULL argument" in lib.gc_last_error().decode()
    assert lib.gc_stream_debug_read_storage(None, 0, 1, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_stream_debug_guards(None, C.byref(front), C.byref(back)) == gnsscorr.GC_ERR_INVALID
    assert "gc_stream_debug_guards: NULL argument" in lib.gc_last_error().decode()
    assert lib.gc_stream_debug_guards(None, None, None) == gnsscorr.GC_ERR_INVALID
    assert (front.value, back.value) == (7, 7)  # nothing is reported for a call that was refused
