"""CPU tests (no GPU) of the CAF engine's C ABI (gc_acq_create_caf, gc_acq_set_local_code_iq, gc_acq_caf_vectors): the symbols are
declared, exported and bound, the header stays C and C++, and every refusal of gc_acq_create_caf answers GC_ERR_INVALID before a
context is looked at (the parameter checks come first, so a NULL context reaches them).  The refusals that need a handle -- the other
engines' setters on a CAF handle, gc_acq_set_local_code_iq on any other -- are made by tests/test_caf_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gc_acq_create_caf", "gc_acq_set_local_code_iq", "gc_acq_caf_vectors")


def test_new_symbols_are_declared_exported_and_bound():
    import gnsscorr
    lib = gnsscorr.load_library()
    txt = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(lib, name), name
        assert name in gnsscorr.API, name
    for m in ("set_local_code_iq", "caf_vectors"):
        assert hasattr(gnsscorr.PcpsAcquisition, m), m
    assert (gnsscorr.CAF_REFERENCE, gnsscorr.CAF_EXACT) == (0, 1)
    assert gnsscorr.PcpsAcquisition.CAF_ARITHMETIC == {"reference": 0, "exact": 1}


def test_header_compiles_as_c_and_cpp(tmp_path):
    src = ('#include "gnsscorr.h"\n'
        "typedef char a_[GC_CAF_REFERENCE == 0 && GC_CAF_EXACT == 1 ? 1 : -1];\n"
        "int use(gc_ctx* c, const gc_acq_conf* f, gc_acq** a, const float* i, const float* q, float* v, uint8_t* b)\n"
        "{ return (int)gc_acq_create_caf(c, f, 1, 1, 2, 3000u, GC_CAF_EXACT, a) + (int)gc_acq_set_local_code_iq(*a, 0, i, q) + (int)gc_acq_caf_vectors(*a, 0, v, v, v, b); }\n")
    for name, cc, std in (("t.c", "gcc", "-std=c99"), ("t.cpp", "g++", "-std=c++14")):
        f = tmp_path / name
        f.write_text(src)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(f), "-o", str(tmp_path / (name + ".o"))])


def _conf(**kw):
    import gnsscorr
    d = dict(fs_in=10000000, sampled_ms=3, ms_per_code=1, samples_per_ms=10000.0, samples_per_code=10000.0, samples_per_chip=1, doppler_max=5000, doppler_step=250, max_dwells=1,
        bit_transition_flag=0, use_cfar=0, override=0, make_2_steps=0, bins2=4, step2=125.0)
    d.update(kw)
    return gnsscorr.AcqConf(*d.values())


REFUSALS = [
    # conf changes, (both_components, hypotheses, caf_window_hz, arithmetic), a word of the message
    ({}, (1, 0, 0, 0), "hypotheses"),
    ({}, (1, 3, 0, 0), "hypotheses"),
    ({}, (2, 2, 0, 0), "both_components"),
    ({}, (1, 2, 0, 2), "arithmetic"),
    ({}, (1, 2, 0, -1), "arithmetic"),
    (dict(doppler_step=0), (1, 2, 0, 0), "doppler_step"),
    (dict(make_2_steps=1), (1, 2, 0, 0), "second step"),
    (dict(bit_transition_flag=1, max_dwells=0), (1, 2, 0, 0), "max_dwells"),
    ({}, (1, 2, 499, 0), "window"),              # H == 0: 0.5 / H
    ({}, (1, 2, 42 * 250, 0), "window"),         # H = 21 needs 43 bins, the grid has 41
    (dict(doppler_max=10000, doppler_step=4), (1, 2, 0, 0), "bins"),  # 5001 bins
    ({}, (1, 2, 0, 0), "NULL context"),          # everything in order: only the context is missing
    ({}, (1, 2, 40 * 250, 0), "NULL context"),   # H = 20 on 41 bins: the largest window the grid admits
    (dict(doppler_max=10000, doppler_step=10), (1, 2, 100, 0), "NULL context"),  # 2001 bins are inside the limit
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_create_refusals_need_no_device(i):
    import gnsscorr
    lib = gnsscorr.load_library()
    conf_kw, (both, hyp, window, arithmetic), word = REFUSALS[i]
    conf = _conf(**conf_kw)
    h = C.c_void_p()
    assert lib.gc_acq_create_caf(None, C.byref(conf), 1, both, hyp, window, arithmetic, C.byref(h)) == gnsscorr.GC_ERR_INVALID
    assert word.encode() in lib.gc_last_error(), lib.gc_last_error()
    assert not h.value


def test_null_arguments_and_the_binding():
    import gnsscorr
    lib = gnsscorr.load_library()
    conf = _conf()
    assert lib.gc_acq_create_caf(None, None, 1, 1, 2, 0, 0, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_create_caf(None, C.byref(conf), 1, 1, 2, 0, 0, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_set_local_code_iq(None, 0, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_caf_vectors(None, 0, None, None, None, None) == gnsscorr.GC_ERR_INVALID
    kw = dict(fs_in=2000000, sampled_ms=2, ms_per_code=1, samples_per_ms=2000.0, samples_per_code=2000.0, samples_per_chip=1, doppler_max=1000, doppler_step=500)
    # caf together with another engine never reaches the library; unknown keys neither
    for other in (dict(combine="max"), dict(folding_factor=2), dict(tong=(1, 2, 3))):
        with pytest.raises(ValueError):
            gnsscorr.PcpsAcquisition(None, 1, caf=dict(hypotheses=2), **kw, **other)
    with pytest.raises(ValueError):
        gnsscorr.PcpsAcquisition(None, 1, caf=dict(hypothesis=2), **kw)
    # an unknown arithmetic name reaches the library and is refused there
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        gnsscorr.PcpsAcquisition(None, 1, caf=dict(arithmetic="fast"), **kw)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID and "arithmetic" in str(ei.value)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        gnsscorr.PcpsAcquisition(None, 1, caf=dict(both_components=1, hypotheses=2, window_hz=1000), **kw)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID and "NULL context" in str(ei.value)


def test_host_side_pieces_of_the_adapter():
    """Keys and defaults, the 3 ms and the zero-padded replica layouts, the threshold rule and the failure path of the C++ adapter, in
    a stand-alone program that creates no GPU context."""
    d = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter")
    subprocess.check_call(["make", "-s", "-C", d, "caf_selftest"])
    p = subprocess.run([os.path.join(d, "caf_selftest"), "--host"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "caf host self-test passed" in p.stdout, p.stdout + p.stderr
