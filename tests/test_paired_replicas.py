"""CPU tests (no GPU) of the paired acquisition engine's host-side pieces: the new entry points are declared and exported, the
two replica helpers equal their numpy statements exactly (codes are +-1), and the identity the CCCWSR mapping rests on --
|d + jp|^2 and |d - jp|^2 of pcps_cccwsr_acquisition_cc.cc:342-351 are the |.|^2 of the correlations with cd - j cp and
cd + j cp -- holds in float64 to 1e-12 of the peak."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gc_acq_create_paired", "gc_acq_set_local_code_pair", "gc_cccwsr_replicas", "gc_e1_8ms_replicas")


def test_new_symbols_are_declared_and_exported():
    import gnsscorr
    txt = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = gnsscorr.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bgc_status\s+%s\s*\(" % name, txt), "%s is not declared in gnsscorr.h" % name
        assert hasattr(lib, name), "libgnsscorr.so does not export %s" % name
        assert name in gnsscorr.API
    assert re.search(r"GC_ACQ_COMBINE_MAX\s*=\s*1\b", txt) and re.search(r"GC_ACQ_COMBINE_SUM\s*=\s*2\b", txt)
    assert gnsscorr.PcpsAcquisition.COMBINE == {"max": 1, "sum": 2}


def test_null_arguments_are_refused_without_a_gpu():
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_acq_create_paired(None, None, 1, 1, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_acq_set_local_code_pair(None, 0, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_cccwsr_replicas(None, None, 4, None, None) == gnsscorr.GC_ERR_INVALID
    assert lib.gc_e1_8ms_replicas(None, 4, 2, None, None) == gnsscorr.GC_ERR_INVALID


def _pm1(rng, n):
    return (2.0 * rng.integers(0, 2, n) - 1.0).astype(np.float32)


def test_cccwsr_replicas_equal_numpy_exactly():
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(11))
    n = 4001
    cd = (_pm1(rng, n) + 0j).astype(np.complex64)
    cp = (_pm1(rng, n) + 0j).astype(np.complex64)
    a, b = gnsscorr.cccwsr_replicas(cd, cp)
    assert a.dtype == np.complex64 and b.dtype == np.complex64
    assert np.array_equal(a, (cd - 1j * cp).astype(np.complex64)) and np.array_equal(b, (cd + 1j * cp).astype(np.complex64))
    # complex +-1 components (an E5a-shaped code): still exact
    cd = (_pm1(rng, n) + 1j * _pm1(rng, n)).astype(np.complex64)
    cp = (_pm1(rng, n) + 1j * _pm1(rng, n)).astype(np.complex64)
    a, b = gnsscorr.cccwsr_replicas(cd, cp)
    assert np.array_equal(a, (cd - 1j * cp).astype(np.complex64)) and np.array_equal(b, (cd + 1j * cp).astype(np.complex64))


def test_e1_8ms_replicas_negate_the_second_code_period_only():
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(12))
    spc = 1000
    one = (_pm1(rng, spc) + 0j).astype(np.complex64)
    for periods in (2, 3):
        code = np.tile(one, periods)
        a, b = gnsscorr.e1_8ms_replicas(code, spc)
        want = code.copy()
        want[spc:2 * spc] = -want[spc:2 * spc]  # galileo_pcps_8ms_acquisition_cc.cc:158-160
        assert np.array_equal(a, code) and np.array_equal(b, want)
    try:
        gnsscorr.e1_8ms_replicas(one, spc)  # one period: no second one to negate
    except gnsscorr.GnsscorrError as e:
        assert e.status == gnsscorr.GC_ERR_INVALID
    else:
        raise AssertionError("a code of one period was accepted")


def test_cccwsr_hypotheses_are_two_complex_replicas_in_float64():
    """One N = 4000 block: |IFFT(X conj FFT(A))|^2 and its B counterpart against the block's own |d + jp|^2 and |d - jp|^2."""
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(13))
    n = 4000
    cd = _pm1(rng, n).astype(np.complex64)
    cp = _pm1(rng, n).astype(np.complex64)
    x = 0.3 * (np.roll(cd, 777) - 1j * np.roll(cp, 777)) * np.exp(2j * np.pi * 0.00005 * np.arange(n)) \
        + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    X = np.fft.fft(x.astype(np.complex128))
    d = np.fft.ifft(X * np.conj(np.fft.fft(cd.astype(np.complex128)))) * n   # unnormalised, as FFTW's backward transform
    p = np.fft.ifft(X * np.conj(np.fft.fft(cp.astype(np.complex128)))) * n
    # pcps_cccwsr_acquisition_cc.cc:342-351
    plus = (d.real - p.imag) + 1j * (d.imag + p.real)
    minus = (d.real + p.imag) + 1j * (d.imag - p.real)
    a, b = gnsscorr.cccwsr_replicas(cd, cp)
    ga = np.abs(np.fft.ifft(X * np.conj(np.fft.fft(a.astype(np.complex128)))) * n) ** 2
    gb = np.abs(np.fft.ifft(X * np.conj(np.fft.fft(b.astype(np.complex128)))) * n) ** 2
    peak = max(ga.max(), gb.max())
    assert np.max(np.abs(ga - np.abs(plus) ** 2)) <= 1e-12 * peak
    assert np.max(np.abs(gb - np.abs(minus) ** 2)) <= 1e-12 * peak
    # the signal is cd - j cp, replica A itself: the plus hypothesis wins, at the signal's delay
    assert ga.max() > 2.0 * gb.max() and int(np.argmax(ga)) == 777
