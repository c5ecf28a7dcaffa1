#!/usr/bin/env python3
"""Generates tests/golden/ref_loop_maths.npz: inputs and outputs of the loop maths of dll_pll_veml_tracking that
oracle/_ref/libref_loop.so compiles from the reference's own files behind the two stand-in headers of oracle/shim
(`make -C oracle ref`; BUILD container only):

  Tracking_loop_filter   src/algorithms/tracking/libs/tracking_loop_filter.cc -- the code loop filter, built with
                         include_last_integrator = false (dll_pll_veml_tracking.cc:340) and re-designed for the narrow stage by
                         set_update_interval then set_noise_bandwidth, without initialize (:1750-1751)
  discriminators         tracking_discriminators.cc:49-128 (run_dll_pll, :914-973)
  lock detectors         lock_detectors.cc:68-111 (cn0_and_tracking_lock_status, :839-878)

Code filter scripts: orders 1, 2, 3 x the five (bandwidth, T wide, narrow bandwidth, T narrow) sets of the carrier filter's scripts
(make_golden_loop.py), 256 steps, the re-design at three quarters.  Discriminators: seeded tap sets VE E P L VL and a previous prompt
at the magnitudes the closed-loop tests produce (prompt about 700, noise about 70 per tap), then edges: P.real == 0, E = L = 0, all
four VEMLP taps zero, negative real prompts, taps of 1e-20 and 1e15.  Lock detectors: prompt buffers of 10 and 20, coherent times
0.001, 0.003 and 0.02 s, a buffer of one constant real value (Ptot - Psig == 0) and an all-zero one (NaN).
The file holds arrays only."""
import ctypes as C
import io
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
fp = C.POINTER(C.c_float)

# (bandwidth, T wide, narrow bandwidth, T narrow)
FILTER_SETS = ((40.0, 0.001, 20.0, 0.020), (15.0, 0.004, 10.0, 0.012), (25.0, 0.001, 15.0, 0.010), (2.0, 0.001, 0.0, 0.001), (40.0, 0.001, 10.0, 0.005))
N_STEPS = 256
COH_TIMES = (0.001, 0.003, 0.02)


def load():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_loop.so"))
    L.ref_lf_new.restype = C.c_void_p
    L.ref_lf_new.argtypes = [C.c_float, C.c_float, C.c_int]
    L.ref_lf_delete.argtypes = [C.c_void_p]
    L.ref_lf_initialize.argtypes = [C.c_void_p]
    L.ref_lf_set_noise_bandwidth.argtypes = [C.c_void_p, C.c_float]
    L.ref_lf_set_update_interval.argtypes = [C.c_void_p, C.c_float]
    L.ref_lf_apply.argtypes = [C.c_void_p, C.c_float]
    L.ref_lf_apply.restype = C.c_float
    L.ref_fll_four_quadrant_atan.argtypes = [fp, fp, C.c_double, C.c_double]
    L.ref_pll_four_quadrant_atan.argtypes = [fp]
    L.ref_pll_cloop_two_quadrant_atan.argtypes = [fp]
    L.ref_dll_nc_e_minus_l_normalized.argtypes = [fp, fp]
    L.ref_dll_nc_vemlp_normalized.argtypes = [fp, fp, fp, fp]
    for n in ("fll_four_quadrant_atan", "pll_four_quadrant_atan", "pll_cloop_two_quadrant_atan", "dll_nc_e_minus_l_normalized", "dll_nc_vemlp_normalized"):
        getattr(L, "ref_" + n).restype = C.c_double
    L.ref_cn0_svn_estimator.argtypes = [fp, C.c_int, C.c_double]
    L.ref_cn0_svn_estimator.restype = C.c_float
    L.ref_carrier_lock_detector.argtypes = [fp, C.c_int]
    L.ref_carrier_lock_detector.restype = C.c_float
    return L


def tap_sets(rng):
    """(n, 6) complex64: VE E P L VL and the previous prompt."""
    n = 512
    noise = (rng.standard_normal((n, 6)) + 1j * rng.standard_normal((n, 6))) * 70.0
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, n))[:, None]
    shape = np.array([0.4, 0.85, 1.0, 0.85, 0.4, 1.0])[None, :] * (700.0 * rng.uniform(0.2, 3.0, n))[:, None]
    t = (shape * phase + noise).astype(np.complex64)
    t[:, 5] *= np.exp(1j * rng.uniform(-0.3, 0.3, n)).astype(np.complex64)
    edges = []

    def edge(ve, e, p, l, vl, po):
        edges.append([ve, e, p, l, vl, po])

    edge(10 + 3j, 50 - 20j, 0 + 700j, 48 + 11j, 9 - 2j, 650 + 20j)        # P.real == 0: the two-quadrant branch returns 0
    edge(10 + 3j, 50 - 20j, 0 - 700j, 48 + 11j, 9 - 2j, -650 - 20j)
    edge(1 + 1j, 2 + 2j, 0 + 0j, 2 - 2j, 1 - 1j, 0 + 0j)                   # P = 0, previous prompt 0: atan2(0, 0)
    edge(30 + 4j, 0 + 0j, 700 + 12j, 0 + 0j, 31 - 5j, 700 - 12j)           # E = L = 0
    edge(0 + 0j, 0 + 0j, 700 + 12j, 0 + 0j, 0 + 0j, 0 + 0j)                # all four VEMLP taps zero
    edge(0 + 0j, 0 + 0j, 0 + 0j, 0 + 0j, 0 + 0j, 0 + 0j)                   # an all-zero input
    edge(-200 + 30j, -500 + 80j, -700 + 90j, -480 + 70j, -190 + 20j, -690 + 60j)   # negative real prompt
    edge(-200 - 30j, -500 - 80j, -700 - 90j, -480 - 70j, -190 - 20j, 690 + 60j)    # ... and a half-cycle jump for the FLL
    edge(-200 + 30j, -500 + 80j, -700 + 0j, -480 + 70j, -190 + 20j, -690 + 0j)     # negative real axis: atan2(+0, -x), cross = 0
    edge(1e-20 + 1e-20j, 1e-20 - 1e-20j, 1e-20 + 1e-20j, 1e-20 + 0j, 0 + 1e-20j, 1e-20 - 1e-20j)  # float norms underflow to denormals / 0
    edge(3e-20 + 1e-20j, 1e-20 - 2e-20j, 2e-20 + 1e-20j, 1e-20 + 1e-20j, 2e-20 + 1e-20j, 1e-20 - 1e-20j)
    edge(1e15 + 1e15j, 1e15 - 2e15j, 1e15 + 3e15j, 2e15 + 1e15j, 1e15 + 1e15j, 1e15 - 1e15j)      # float norms of 1e30
    edge(1e15 + 1e15j, 1e-20 - 1e-20j, 1e15 + 1e-20j, 1e15 + 1e15j, 1e-20 + 1e-20j, 1e-20 + 1e15j)
    return np.concatenate([t, np.array(edges, np.complex64)])


def prompt_buffers(rng, length):
    """(n, length) complex64 prompt buffers and their coherent times."""
    n = 240
    sign = rng.integers(0, 2, (n, length)) * 2.0 - 1.0
    amp = (700.0 * rng.uniform(0.05, 3.0, n))[:, None]
    ph = np.exp(1j * rng.uniform(-0.5, 0.5, n))[:, None]
    b = (sign * amp * ph + (rng.standard_normal((n, length)) + 1j * rng.standard_normal((n, length))) * 70.0).astype(np.complex64)
    extra = np.zeros((4, length), np.complex64)
    extra[0, :] = 123.5            # one constant real value: Ptot - Psig == 0
    extra[1, :] = -0.75
    # extra[2]: all zero (0 / 0)
    extra[3, :] = 5 + 300j         # mostly quadrature: a negative lock test, Ptot far above Psig
    b = np.concatenate([b, extra])
    T = np.array([COH_TIMES[k % 3] for k in range(len(b))], np.float64)
    return b, T


def main():
    L = load()
    rng = np.random.Generator(np.random.PCG64(20261021))
    out = {}
    i = 0
    for order in (1, 2, 3):
        for bw, t_wide, narrow, t_narrow in FILTER_SETS:
            e = (rng.standard_normal(N_STEPS) * 0.05 + 0.03 * np.cos(np.arange(N_STEPS) / 23.0)).astype(np.float32)
            n_switch = 3 * N_STEPS // 4
            f = L.ref_lf_new(t_wide, bw, order)
            L.ref_lf_initialize(f)
            y = np.zeros(N_STEPS, np.float32)
            for k in range(N_STEPS):
                if k == n_switch:  # the block's order (:1750-1751)
                    L.ref_lf_set_update_interval(f, t_narrow)
                    L.ref_lf_set_noise_bandwidth(f, narrow)
                y[k] = L.ref_lf_apply(f, float(e[k]))
            L.ref_lf_delete(f)
            out["lf%d_conf" % i] = np.array([order, bw, t_wide, narrow, t_narrow, n_switch], np.float64)
            out["lf%d_in" % i], out["lf%d_out" % i] = e, y
            i += 1
    out["n_lf"] = np.int64(i)

    taps = np.ascontiguousarray(tap_sets(rng))
    T = np.array([COH_TIMES[k % 3] for k in range(len(taps))], np.float64)
    res = {k: np.zeros(len(taps), np.float64) for k in ("fll", "pll4", "pll2", "eml", "vemlp")}
    for k in range(len(taps)):
        p = [taps[k, j:j + 1].view(np.float32).ctypes.data_as(fp) for j in range(6)]
        res["fll"][k] = L.ref_fll_four_quadrant_atan(p[5], p[2], 0.0, T[k])
        res["pll4"][k] = L.ref_pll_four_quadrant_atan(p[2])
        res["pll2"][k] = L.ref_pll_cloop_two_quadrant_atan(p[2])
        res["eml"][k] = L.ref_dll_nc_e_minus_l_normalized(p[1], p[3])
        res["vemlp"][k] = L.ref_dll_nc_vemlp_normalized(p[0], p[1], p[3], p[4])
    out["disc_taps"], out["disc_T"] = taps, T
    for k, v in res.items():
        out["disc_" + k] = v

    for length in (10, 20):
        b, Tb = prompt_buffers(rng, length)
        b = np.ascontiguousarray(b)
        cn0, lock = np.zeros(len(b), np.float32), np.zeros(len(b), np.float32)
        for k in range(len(b)):
            ptr = b[k].view(np.float32).ctypes.data_as(fp)
            cn0[k] = L.ref_cn0_svn_estimator(ptr, length, Tb[k])
            lock[k] = L.ref_carrier_lock_detector(ptr, length)
        out["lock%d_in" % length], out["lock%d_T" % length], out["lock%d_cn0" % length], out["lock%d_test" % length] = b, Tb, cn0, lock

    path = os.path.join(HERE, "ref_loop_maths.npz")
    # an .npz with fixed member dates, so that a regenerated file is the committed one byte for byte
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes;", i, "code filter scripts,", len(taps), "tap sets,", "2 x", len(b), "prompt buffers")


if __name__ == "__main__":
    main()
