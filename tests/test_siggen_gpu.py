"""GPU tests of the signal generator stage (gc_signal_generator_*, gnss-sdr-1_amd/csrc/siggen_kernels.hip): the device's samples
against the numpy restatement of the model (tests/siggen_ref.py), bit-for-bit independence of how the stream is cut into calls,
pieces and tiles, 64-bit sample numbers, the noise's statistics, the integer rings, and the source feeding acquisition and the
closed tracking loop with no host link in between.

The parity gate, max |dev - ref| <= 1e-5 A + 2e-5 sigma with A = sum_s amplitude_s sum_c |gain_c| max |table_c|, is derived:
  signal  an angle carried as float32 turns is off by at most 2 pi 2^-24 = 3.7e-7, sincos by a few 1e-7, each product and each of
          up to 32 accumulations by at most 2^-24 relative: under 2e-6 A in all, gated with 5x margin (32 satellites are
          actually run, with every signal kind and both axes, in tests/test_siggen_matrix_gpu.py)
  noise   r <= 5.77 with relative error near 2e-7, 2 pi u2 rounded to float32 gives 3.7e-7 x 5.77: about 4e-6 sigma, 5x margin"""
import numpy as np
import pytest

import conditioner_out_ref as out_ref
import siggen_cases as cases
import siggen_ref as ref

pytestmark = pytest.mark.gpu
FS, N = cases.FS, cases.N
TOTAL = 30001


def _gate(scene, sigma):
    return 1e-5 * ref.amplitude_bound(scene["dicts"]) + 2e-5 * sigma


@pytest.fixture(scope="module")
def scene():
    """The shared scene, and the restatement's 30001 samples of it, with and without noise: computed once, never changed."""
    import gnsscorr
    sats, sigma, seed = cases.shared_scene(gnsscorr)
    dicts = [ref.from_satellite(s, FS) for s in sats]
    clean = ref.generate(dicts, 0.0, seed, 0, TOTAL)
    noisy = clean + float(np.float32(sigma)) * ref.noise(seed, 0, TOTAL)
    for a in (clean, noisy):
        a.setflags(write=False)
    return dict(sats=sats, sigma=sigma, seed=seed, dicts=dicts, clean=clean, noisy=noisy)


def _generate(gctx, scene, calls, capacity, sigma, iq_format=None, scale=None, t0=0, max_window=4000, placement="auto"):
    import gnsscorr
    fmt = gnsscorr.GC_IQ_F32 if iq_format is None else iq_format
    ring = gnsscorr.IqStream(gctx, capacity_samples=capacity, max_window_samples=max_window, iq_format=fmt)
    if fmt != gnsscorr.GC_IQ_F32:
        ring.accept_quantised_output()
    gen = gnsscorr.SignalGenerator(gctx, ring, scene.get("fs", FS), scene["sats"], noise_sigma=sigma, seed=scene["seed"], t0=t0, table_placement=placement)
    if scale is not None:
        gen.set_output_scale(scale)
    head = 0
    for n in calls:
        assert gen.generate(n) == head
        head += n
    assert gen.info() == head and ring.info()[1] == head
    return ring, gen


@pytest.mark.parametrize("noise", [False, True])
def test_parity_with_the_restatement(gctx, scene, noise):
    sigma = scene["sigma"] if noise else 0.0
    ring, gen = _generate(gctx, scene, [11999], 12000, sigma)
    dev = ring.read(0, 11999)
    want = scene["noisy" if noise else "clean"][:11999]
    err = float(np.max(np.abs(dev.astype(np.complex128) - want)))
    print("parity, noise %s: max |dev - ref| = %.3e, gate %.3e (A = %.4f, sigma = %.4f)" % (noise, err, _gate(scene, sigma),
        ref.amplitude_bound(scene["dicts"]), sigma))
    assert dev.dtype == np.complex64 and err <= _gate(scene, sigma)
    assert np.abs(want).max() > 0.5  # the scene is not silence
    gen.close()
    ring.close()


def _window_sum(gctx, ring, first, n):
    """A correlator with an all-ones replica over [first, first + n): a window across the ring's end is read through the mirror."""
    import gnsscorr
    b = gnsscorr.TrackingBatch(gctx, 1, 3, 8)
    b.set_code(0, np.ones(8, np.float32), np.zeros(3, np.float32))
    b.set_input_stream(0, ring)
    got = b.run(1, gnsscorr.epoch_params_array([gnsscorr.epoch_params(first, 0.0, 0.0, 0.0, 0.001, n)]))[0, 0, 1]
    b.close()
    return np.complex64(got)


def test_partition_and_wrap_independence_bit_for_bit(gctx, scene):
    """Two generators of the same scene on rings of 12000 samples (max_window 4000): A appends 30001 samples in calls of 11999, 12000
    and 6002, B in calls of 1, 7, 4093, 3898, 4000, 12001 and 6001 -- an odd start that splits a 16-byte store, a call longer than
    the ring, the wrap and the mirror crossed several times.  What the rings hold at the end is byte-identical, and is the
    restatement's within the parity gate."""
    sigma = scene["sigma"]
    ring_a, gen_a = _generate(gctx, scene, [11999, 12000, 6002], 12000, sigma)
    ring_b, gen_b = _generate(gctx, scene, [1, 7, 4093, 3898, 4000, 12001, 6001], 12000, sigma)
    a, b = ring_a.read(TOTAL - 12000, 12000), ring_b.read(TOTAL - 12000, 12000)
    assert a.tobytes() == b.tobytes()
    err = float(np.max(np.abs(a.astype(np.complex128) - scene["noisy"][TOTAL - 12000:])))
    print("partition: max |dev - ref| = %.3e over the resident 12000, gate %.3e" % (err, _gate(scene, sigma)))
    assert err <= _gate(scene, sigma)
    # [23000, 25000) spans the ring's end (sample 24000 is at position 0): contiguous only through the mirror the kernel stored
    wrap = 24000
    across_a, across_b = ring_a.read(wrap - 1000, 2000), ring_b.read(wrap - 1000, 2000)
    assert across_a.tobytes() == across_b.tobytes()
    sum_a, sum_b = _window_sum(gctx, ring_a, wrap - 1000, 2000), _window_sum(gctx, ring_b, wrap - 1000, 2000)
    assert sum_a.tobytes() == sum_b.tobytes()
    want = across_a.astype(np.complex128).sum()
    tol = (2000 + 8) * 2.0 ** -24 * np.abs(across_a).sum() * np.sqrt(2.0)  # the correlator's own float32 sum of 2000 stored values
    assert abs(complex(sum_a) - want) <= tol and np.abs(across_a[1000:]).sum() > 100 * tol  # a stale mirror would be far outside
    for h in (gen_a, gen_b, ring_a, ring_b):
        h.close()


def test_sample_numbers_beyond_32_bits(gctx, scene):
    t0 = (1 << 40) + 12345
    ring, gen = _generate(gctx, scene, [4093], 12000, scene["sigma"], t0=t0)
    dev = ring.read(0, 4093)
    want = ref.generate(scene["dicts"], scene["sigma"], scene["seed"], t0, 4093)
    err = float(np.max(np.abs(dev.astype(np.complex128) - want)))
    print("t0 = 2^40 + 12345: max |dev - ref| = %.3e, gate %.3e" % (err, _gate(scene, scene["sigma"])))
    assert err <= _gate(scene, scene["sigma"])
    # and it is another stretch of the scene than the one that starts at 0
    assert np.max(np.abs(dev.astype(np.complex128) - scene["noisy"][:4093])) > 0.5
    gen.close()
    ring.close()


def test_tables_in_lds_give_the_same_bits(gctx):
    """The table placement is a matter of speed alone: the GPS satellites of the acquisition scene (4 x 1023 entries fit in LDS)
    from HBM and from LDS, byte for byte."""
    import gnsscorr
    sats, sigma, seed = cases.acquisition_scene(gnsscorr)
    small = dict(sats=sats, seed=seed)
    got = {}
    for placement in ("hbm", "lds"):
        ring, gen = _generate(gctx, small, [4093, 3000], 8192, sigma, placement=placement, max_window=1000)
        got[placement] = ring.read(0, 7093).tobytes()
        gen.close()
        ring.close()
    assert got["hbm"] == got["lds"]


def test_noise_statistics(gctx):
    """2^20 samples of noise alone (one satellite of amplitude 0), sigma 1, seed 5: five standard deviations of each estimator;
    test_siggen_ref.py asserts the same of the restatement with the same seed."""
    import gnsscorr
    n = 1 << 20
    silent = gnsscorr.SiggenSatellite(0.0, 1.0 / N, [dict(table=np.ones(1023, np.float32))], amplitude=0.0)
    ring, gen = _generate(gctx, dict(sats=[silent], seed=5), [n], n, 1.0, max_window=N)
    g = ring.read(0, n).astype(np.complex128)
    gen.close()
    ring.close()
    re, im = g.real, g.imag
    figures = dict(mean_re=re.mean(), mean_im=im.mean(), var_re=re.var() - 1.0, var_im=im.var() - 1.0, corr=np.mean(re * im),
        lag1_re=np.mean(re[1:] * re[:-1]), lag1_im=np.mean(im[1:] * im[:-1]))
    print("noise statistics over 2^20 samples:", {k: "%.2e" % v for k, v in figures.items()}, "bounds %.2e / %.2e" % (5 / np.sqrt(n), 5 * np.sqrt(2.0 / n)))
    for part in (re, im):
        assert abs(part.mean()) <= 5 / np.sqrt(n)
        assert abs(part.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
        assert abs(np.mean(part[1:] * part[:-1])) <= 5 / np.sqrt(n)
    assert abs(np.mean(re * im)) <= 5 / np.sqrt(n)
    # the device's noise is the restatement's: the first 4096 samples within the noise part of the gate
    assert np.max(np.abs(g[:4096] - ref.noise(5, 0, 4096))) <= 2e-5


@pytest.mark.parametrize("fmt_name, scale", [("GC_IQ_I16", 20000.0), ("GC_IQ_I8", 100.0)])
def test_integer_rings_are_the_epilogue_of_the_float_ring(gctx, scene, fmt_name, scale):
    """The same scene into an integer ring of 5001 samples (odd: the mirror's dword boundaries differ from the ring's) in calls
    of odd sizes: every component is the restated epilogue applied to the F32 ring's own device output -- the same floats in, so
    exactly -- and the clipped count is the restatement's.  The scales clip some components and only some."""
    import gnsscorr
    fmt = getattr(gnsscorr, fmt_name)
    sigma = scene["sigma"]
    ring_f, gen_f = _generate(gctx, scene, [11999], 12000, sigma)
    y = ring_f.read(0, 11999)
    gen_f.close()
    ring_f.close()
    ring, gen = _generate(gctx, scene, [1, 4093, 7905], 5001, sigma, iq_format=fmt, scale=scale, max_window=1000)
    got = ring.read(11999 - 5001, 5001)
    want, clipped = out_ref.quantise(y, fmt, scale)
    assert got.tobytes() == want[11999 - 5001:].tobytes()
    out_format, out_scale, n_clipped = gen.output_info()
    print("%s: %d of %d components clipped at scale %g" % (fmt_name, n_clipped, 2 * 11999, scale))
    assert (out_format, out_scale, n_clipped) == (fmt, scale, clipped)
    assert 0 < clipped < 2 * 11999 // 4
    # a window across the ring's end, [9500, 10500) (sample 10002 is at position 0), is read through the mirror: a correlator gives
    # the bits it gives on a ring of the same size into which the host pushed the restated integers
    pushed = gnsscorr.IqStream(gctx, capacity_samples=5001, max_window_samples=1000, iq_format=fmt)
    for first in range(0, 11999, 4000):
        pushed.push(want[first:first + 4000])
    sums = []
    for r in (ring, pushed):
        b = gnsscorr.TrackingBatch(gctx, 1, 3, 8)
        b.set_input_format(fmt)
        b.set_code(0, np.ones(8, np.float32), np.zeros(3, np.float32))
        b.set_input_stream(0, r)
        sums.append(b.run(1, gnsscorr.epoch_params_array([gnsscorr.epoch_params(9500, 0.0, 0.0, 0.0, 0.001, 1000)]))[0, 0].copy())
        b.close()
    pushed.close()
    assert sums[0].tobytes() == sums[1].tobytes() and abs(sums[0][1]) > 0.0
    with pytest.raises(gnsscorr.GnsscorrError, match="generated already"):
        gen.set_output_scale(1.0)
    gen.close()
    ring.close()


def test_life_cycle_of_the_ring_claim(gctx, scene):
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=8000, max_window_samples=1000)
    gen = gnsscorr.SignalGenerator(gctx, ring, FS, scene["sats"])
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        ring.push(np.zeros(16, np.complex64))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.SignalGenerator(gctx, ring, FS, scene["sats"])
    assert e.value.status == gnsscorr.GC_ERR_STATE and "already has a producer" in str(e.value)
    with pytest.raises(gnsscorr.GnsscorrError, match="no scale"):
        gen.set_output_scale(2.0)
    assert gen.output_info() == (gnsscorr.GC_IQ_F32, 1.0, 0)
    gen.close()
    ring.push(np.zeros(16, np.complex64))  # the ring is the host's again
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.SignalGenerator(gctx, ring, FS, scene["sats"])
    assert e.value.status == gnsscorr.GC_ERR_STATE and "pushed into the ring already" in str(e.value)
    plain = gnsscorr.IqStream(gctx, capacity_samples=8000, max_window_samples=1000, iq_format=gnsscorr.GC_IQ_I16)
    with pytest.raises(gnsscorr.GnsscorrError, match="gc_stream_accept_quantised_output"):
        gnsscorr.SignalGenerator(gctx, plain, FS, scene["sats"])
    plain.close()
    ring.close()


def test_source_to_acquisition_without_a_host_link(gctx, oracle):
    """Four GPS satellites at 50 dB-Hz in CN(0, 1) noise, generated into a ring; PCPS over 32 PRNs at N = 4000 straight from it.
    test_siggen_ref.py shows the CPU oracle meeting the same conditions on the restated stream."""
    import gnsscorr
    sats, sigma, seed = cases.acquisition_scene(gnsscorr)
    ring, gen = _generate(gctx, dict(sats=sats, seed=seed), [2 * N], 8 * N, sigma)
    acq = gnsscorr.PcpsAcquisition(gctx, 32, FS, 1, 1, np.float32(FS) * np.float32(0.001), 4000.0, 4, 5000, 250)
    for s in range(32):
        acq.set_local_code(s, oracle.gps_l1_ca_code_sampled(s + 1, FS))
    res = acq.dwell_stream(ring, 0)
    acq.close()
    gen.close()
    ring.close()
    cases.check_acquisition([(float(r.test_statistics), float(r.doppler_hz), float(r.indext)) for r in res])


def test_source_to_closed_loop(gctx, oracle):
    """300 ms of one satellite with data bits and a consistent code Doppler, generated 5 ms at a time into the ring the loop
    tracks on, started from the truth: the PLL settles on the true Doppler and holds lock (the figures of
    tests/test_receiver_flow_gpu.py for this check)."""
    import gnsscorr
    from test_closed_loop_gpu import GPS, _conf
    sats, sigma, seed = cases.tracking_scene(gnsscorr)
    n_ms = 300
    ring = gnsscorr.IqStream(gctx, capacity_samples=40 * N, max_window_samples=4 * N)
    gen = gnsscorr.SignalGenerator(gctx, ring, FS, sats, noise_sigma=sigma, seed=seed)
    gen.generate(4 * N)
    loop = gnsscorr.TrackingLoop(gctx, 1, 1023)
    loop.set_input_stream(0, ring)
    conf = dict(GPS, acq_delay_samples=cases.TRK_DELAY, acq_doppler_hz=cases.TRK_DOPPLER, acq_samplestamp_samples=0, sample_counter=0)
    loop.start(0, _conf(gnsscorr, **conf), oracle.gps_l1_ca_code(cases.TRK_PRN).astype(np.float32))
    recs = []
    for ms in range(4, n_ms, 5):
        gen.generate(5 * N)
        recs.extend(r.copy() for r in loop.run(6)[0] if r["valid"])
    loop.close()
    gen.close()
    ring.close()
    rr = np.array(recs)
    assert len(rr) >= n_ms - 3
    doppler = float(rr["carrier_doppler_hz"][-50:].mean())
    print("closed loop: mean carrier Doppler of the last 50 periods %.2f Hz (truth %.1f), lock test %.3f" % (doppler, cases.TRK_DOPPLER, rr["carrier_lock_test"][-1]))
    assert abs(doppler - cases.TRK_DOPPLER) < 3.0
    assert rr["carrier_lock_test"][-1] > 0.8
