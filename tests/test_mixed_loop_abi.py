"""CPU tests (no GPU) of the closed-loop engine's mixed mode (gc_trk_loop_set_mixed): the symbol is declared and exported,
a NULL handle is refused without touching a GPU, and the header still compiles as C99."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gnsscorr.h")


def test_set_mixed_is_declared_and_exported():
    import gnsscorr
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"gc_status\s+gc_trk_loop_set_mixed\s*\(\s*gc_trk_loop\s*\*\s*l\s*,\s*int\s+on\s*\)\s*;", txt)
    lib = gnsscorr.load_library()
    assert hasattr(lib, "gc_trk_loop_set_mixed")
    assert "gc_trk_loop_set_mixed" in gnsscorr.API


def test_set_mixed_null_handle_is_invalid_without_gpu():
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_trk_loop_set_mixed(None, 1) == gnsscorr.GC_ERR_INVALID
    assert "gc_trk_loop_set_mixed" in lib.gc_last_error().decode()
    assert lib.gc_trk_loop_set_mixed(None, 0) == gnsscorr.GC_ERR_INVALID


def test_header_with_set_mixed_compiles_as_c99(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include "gnsscorr.h"\n'
                   'static gc_status (*const fn)(gc_trk_loop*, int) = gc_trk_loop_set_mixed;\n'
                   'int main(void){ return fn == 0; }\n')
    obj = str(tmp_path / "m.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", obj])
