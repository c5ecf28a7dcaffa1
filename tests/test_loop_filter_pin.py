"""CPU tests (no GPU): the loop filters of row f1 against the REFERENCE's own filters compiled in oracle/_ref.

tests/golden/ref_loop_filters.npz (tests/golden/make_golden_loop.py, build container) holds scripted call sequences and the
outputs of the reference's Tracking_FLL_PLL_filter (tracking_FLL_PLL_filter.cc:55-133: the carrier loop filter of
dll_pll_veml_tracking, dll_pll_veml_tracking.cc:914-973), Tracking_2nd_DLL_filter and Tracking_2nd_PLL_filter.  Held to them
BIT FOR BIT (float32 bit patterns, 256 steps per script, bandwidth narrowed and correlation time changed mid-script):
  * tests/closed_loop_ref.py::Pll -- the checker of the device loop, so the GPU parity of carrier_doppler_hz rests on a pinned filter;
  * adapter/tracking_loop_maths.h::Tracking_FLL_PLL_filter (the host-loop image) and the second-order filters of
    adapter/hip_glonass_ca_dll_pll_tracking.h, compiled here with g++ -ffp-contract=off like the reference was.
The device loop's own copy (csrc/trk_closed_loop.hip::pll_get_carrier_error) is checked on the GPU against the pinned Pll fed
with the device's recorded discriminator outputs (tests/test_closed_loop_gpu.py::test_device_carrier_filter_against_the_pinned_filter).

tests/golden/ref_loop_maths.npz (tests/golden/make_golden_loop_maths.py) does the same for the rest of the veml loop's maths, compiled
from the reference's tracking_loop_filter.cc, tracking_discriminators.cc and lock_detectors.cc behind the stand-in headers of
oracle/shim: the code loop filter of orders 1 to 3 with its narrow-stage re-design, the five discriminators, the C/N0 estimator and
the carrier lock detector.  closed_loop_ref.py's LoopFilter, lock detectors, E-minus-L and VEMLP are held to it bit for bit (NaN equal
to NaN); its three atan-based discriminators run numpy's arctan / arctan2, another libm than the reference's glibc, and are held to
U_CPU ulp.  The adapter's copies (tracking_loop_maths.h) use glibc like the reference: everything bit for bit.  The device's copies are
checked on the GPU by tests/test_loop_maths_gpu.py, which replays the device's records through the restatement pinned here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
fp = C.POINTER(C.c_float)
dp = C.POINTER(C.c_double)

# The largest distance, in ulp of the function's own type (float32 for the two PLL discriminators, double for the FLL one), that
# numpy's arctan / arctan2 may have from the compiled reference's glibc on the golden inputs.  1 is what two correctly-working libms
# differ by; more would be a wrong restatement, not a reason for a larger constant.  tests/test_loop_maths_gpu.py grants the device's
# libm U_CPU + 2.
U_CPU = 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_python_restatement_of_the_carrier_filter_is_bit_exact():
    from closed_loop_ref import Pll
    z = np.load(os.path.join(G, "ref_loop_filters.npz"))
    assert int(z["n_fll_pll"]) == 15
    for i in range(int(z["n_fll_pll"])):
        order, fll_bw, pll_bw, narrow, dopp, n_switch = z["fp%d_conf" % i]
        f = Pll(float(fll_bw), float(pll_bw), int(order))
        f.initialize(np.float32(dopp))
        fll, pll, T, want = z["fp%d_fll" % i], z["fp%d_pll" % i], z["fp%d_T" % i], z["fp%d_out" % i]
        got = np.zeros(len(want), np.float32)
        for k in range(len(want)):
            if k == int(n_switch):
                f.set_params(float(fll_bw), float(narrow), int(order))
            got[k] = f.get_carrier_error(fll[k], pll[k], T[k])
        assert np.array_equal(_bits(got), _bits(want)), ("script %d (order %d)" % (i, order), np.flatnonzero(_bits(got) != _bits(want))[:5])


@pytest.fixture(scope="module")
def capi(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("capi") / "libloopcapi.so")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-DWITH_SECOND_ORDER",
        "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "adapter"), "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "loop_filter_capi.cpp"), "-o", so,
        "-L", os.path.join(ROOT, "gnss-sdr-1_amd"), "-lgnsscorr", "-Wl,-rpath," + os.path.join(ROOT, "gnss-sdr-1_amd")])
    L = C.CDLL(so)
    L.fp_run.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, fp, fp, fp, fp]
    L.s2_run.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, fp, fp]
    L.lf_run.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, fp, fp]
    L.disc_run.argtypes = [C.c_int, fp, dp, dp]
    L.lock_run.argtypes = [C.c_int, C.c_int, fp, dp, fp, fp]
    return L


def test_adapter_carrier_filter_is_bit_exact(capi):
    z = np.load(os.path.join(G, "ref_loop_filters.npz"))
    for i in range(int(z["n_fll_pll"])):
        order, fll_bw, pll_bw, narrow, dopp, n_switch = z["fp%d_conf" % i]
        fll, pll, T, want = (np.ascontiguousarray(z["fp%d_%s" % (i, k)], np.float32) for k in ("fll", "pll", "T", "out"))
        got = np.zeros_like(want)
        capi.fp_run(int(order), fll_bw, pll_bw, narrow, dopp, int(n_switch), len(want), fll.ctypes.data_as(fp), pll.ctypes.data_as(fp),
            T.ctypes.data_as(fp), got.ctypes.data_as(fp))
        assert np.array_equal(_bits(got), _bits(want)), "script %d (order %d)" % (i, order)


def test_adapter_second_order_filters_are_bit_exact(capi):
    z = np.load(os.path.join(G, "ref_loop_filters.npz"))
    for i in range(int(z["n_second_order"])):
        bw, pdi, bw2, pdi2 = z["s2_%d_conf" % i]
        e = np.ascontiguousarray(z["s2_%d_in" % i], np.float32)
        for which, name in ((0, "dll2"), (1, "pll2")):
            want = z["%s_%d_out" % (name, i)]
            got = np.zeros_like(want)
            capi.s2_run(which, bw, pdi, bw2, pdi2, len(e), e.ctypes.data_as(fp), got.ctypes.data_as(fp))
            assert np.array_equal(_bits(got), _bits(want)), "%s script %d" % (name, i)


# ---- the code loop filter, the discriminators and the lock detectors of the veml loop (tests/golden/ref_loop_maths.npz) ----
def _same(got, want):
    """Bit patterns equal; NaN equals NaN (any payload), which leaves +-inf and +-0 to the bit patterns."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))


def _ulps(got, want):
    """Distance in representable values of the arrays' type; NaN against NaN is 0, NaN against a number is huge."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype
    i = np.int32 if got.dtype == np.float32 else np.int64
    def key(a):
        b = a.view(i).astype(np.int64) if i is np.int32 else a.view(i)
        return np.where(b < 0, np.iinfo(i).min - b, b).astype(object)  # monotone in the value: -0 and +0 coincide
    d = np.abs(key(got) - key(want))
    both = np.isnan(got) & np.isnan(want)
    one = np.isnan(got) ^ np.isnan(want)
    return np.where(both, 0, np.where(one, 2 ** 62, d))


@pytest.fixture(scope="module")
def maths():
    z = np.load(os.path.join(G, "ref_loop_maths.npz"))
    assert int(z["n_lf"]) == 15 and len(z["disc_taps"]) >= 512 + 10
    return z


def test_python_restatement_of_the_code_filter_is_bit_exact(maths):
    from closed_loop_ref import LoopFilter
    z = maths
    orders = set()
    for i in range(int(z["n_lf"])):
        order, bw, t_wide, narrow, t_narrow, n_switch = z["lf%d_conf" % i]
        f = LoopFilter(np.float32(t_wide), np.float32(bw), int(order))
        e, want = z["lf%d_in" % i], z["lf%d_out" % i]
        assert len(want) == 256
        got = np.zeros(len(want), np.float32)
        for k in range(len(want)):
            if k == int(n_switch):
                f.design(np.float32(t_narrow), np.float32(narrow))
            got[k] = f.apply(e[k])
        assert np.all(_same(got, want)), ("script %d (order %d)" % (i, order), np.flatnonzero(~_same(got, want))[:5])
        assert len(np.unique(want)) > 150  # a first-order filter narrowed to a bandwidth of 0 gives zeros in its last quarter
        orders.add(int(order))
    assert orders == {1, 2, 3}


def test_python_restatement_of_the_lock_detectors_is_bit_exact(maths):
    import closed_loop_ref as R
    z = maths
    for length in (10, 20):
        b, T = z["lock%d_in" % length], z["lock%d_T" % length]
        assert b.shape[1] == length and set(T) == {0.001, 0.003, 0.02}
        cn0 = np.array([R.cn0_svn_estimator(b[k], T[k]) for k in range(len(b))], np.float32)
        lock = np.array([R.carrier_lock_detector(b[k]) for k in range(len(b))], np.float32)
        assert np.all(_same(cn0, z["lock%d_cn0" % length])), np.flatnonzero(~_same(cn0, z["lock%d_cn0" % length]))[:5]
        assert np.all(_same(lock, z["lock%d_test" % length])), np.flatnonzero(~_same(lock, z["lock%d_test" % length]))[:5]
        # the edges are in the file: a constant real buffer (SNR = x / 0), an all-zero one (NaN from both detectors)
        assert np.any(np.isinf(z["lock%d_cn0" % length])) and np.any(np.isnan(z["lock%d_cn0" % length])) and np.any(np.isnan(z["lock%d_test" % length]))


def _python_discriminators(z):
    import closed_loop_ref as R
    t, T = z["disc_taps"], z["disc_T"]
    out = {k: np.zeros(len(t), np.float64) for k in ("fll", "pll4", "pll2", "eml", "vemlp")}
    for k in range(len(t)):
        VE, E, P, L, VL, Pold = t[k]
        out["fll"][k] = R.fll_four_quadrant_atan(Pold, P, 0.0, T[k])
        out["pll4"][k] = R.pll_four_quadrant_atan(P)
        out["pll2"][k] = R.pll_cloop_two_quadrant_atan(P)
        out["eml"][k] = R.dll_nc_e_minus_l_normalized(E, L)
        out["vemlp"][k] = R.dll_nc_vemlp_normalized(VE, E, L, VL)
    return out


def test_python_restatement_of_the_code_discriminators_is_bit_exact(maths):
    got = _python_discriminators(maths)
    for k in ("eml", "vemlp"):
        ok = _same(got[k], maths["disc_" + k])
        assert np.all(ok), (k, np.flatnonzero(~ok)[:5], got[k][~ok][:5], maths["disc_" + k][~ok][:5])
    assert np.count_nonzero(maths["disc_vemlp"] == 0.0) >= 2 and np.count_nonzero(maths["disc_eml"] == 0.0) >= 2  # the zero-tap edges


def test_python_restatement_of_the_carrier_discriminators_is_within_one_ulp_of_glibc(maths):
    """numpy's arctan / arctan2 against the reference's glibc: float32 ulp for the two PLL discriminators (float atan / atan2 widened
    to double), double ulp of the atan2 itself for the FLL one: the distance is the smallest shift of the restatement's atan2 result
    that reproduces the golden quotient atan2 / (t2 - t1) bit for bit."""
    z = maths
    got = _python_discriminators(z)
    worst = {}
    for k in ("pll4", "pll2"):
        assert np.array_equal(z["disc_" + k].astype(np.float32).astype(np.float64), z["disc_" + k], equal_nan=True)  # float results
        worst[k] = int(np.max(_ulps(got[k].astype(np.float32), z["disc_" + k].astype(np.float32))))
    import closed_loop_ref as R
    t, T = z["disc_taps"], z["disc_T"]
    need = np.zeros(len(t), np.int64)
    for k in range(len(t)):
        want = z["disc_fll"][k]
        hit = [abs(m) for m in (0, -1, 1, -2, 2) if _same(np.float64(R.fll_four_quadrant_atan(t[k, 5], t[k, 2], 0.0, T[k], move=m)), np.float64(want))]
        need[k] = hit[0] if hit else 99
    worst["fll"] = int(need.max())
    print("numpy against glibc, largest distance [ulp]:", worst)
    assert max(worst.values()) <= U_CPU, worst
    assert U_CPU <= 1


def test_adapter_code_filter_is_bit_exact(capi, maths):
    z = maths
    for i in range(int(z["n_lf"])):
        order, bw, t_wide, narrow, t_narrow, n_switch = z["lf%d_conf" % i]
        e, want = (np.ascontiguousarray(z["lf%d_%s" % (i, k)], np.float32) for k in ("in", "out"))
        got = np.zeros_like(want)
        capi.lf_run(int(order), bw, t_wide, narrow, t_narrow, int(n_switch), len(want), e.ctypes.data_as(fp), got.ctypes.data_as(fp))
        assert np.all(_same(got, want)), "script %d (order %d)" % (i, order)


def test_adapter_discriminators_are_bit_exact(capi, maths):
    z = maths
    t = np.ascontiguousarray(z["disc_taps"], np.complex64)
    T = np.ascontiguousarray(z["disc_T"], np.float64)
    got = np.zeros((len(t), 5), np.float64)
    capi.disc_run(len(t), t.view(np.float32).ctypes.data_as(fp), T.ctypes.data_as(dp), got.ctypes.data_as(dp))
    for j, k in enumerate(("fll", "pll4", "pll2", "eml", "vemlp")):
        ok = _same(np.ascontiguousarray(got[:, j]), z["disc_" + k])
        assert np.all(ok), (k, np.flatnonzero(~ok)[:5])


def test_adapter_lock_detectors_are_bit_exact(capi, maths):
    z = maths
    for length in (10, 20):
        b = np.ascontiguousarray(z["lock%d_in" % length], np.complex64)
        T = np.ascontiguousarray(z["lock%d_T" % length], np.float64)
        cn0, lock = np.zeros(len(b), np.float32), np.zeros(len(b), np.float32)
        capi.lock_run(len(b), length, b.view(np.float32).ctypes.data_as(fp), T.ctypes.data_as(dp), cn0.ctypes.data_as(fp), lock.ctypes.data_as(fp))
        assert np.all(_same(cn0, z["lock%d_cn0" % length])) and np.all(_same(lock, z["lock%d_test" % length])), length
