"""CPU tests (no GPU) of the signal generator's model: the numpy restatement (tests/siggen_ref.py) against the Philox known answers,
the C ABI's conversion rule, the library's own sampled L1 C/A generator and the detection conditions the GPU tests assert -- so
that whatever those tests find on the device is judged against arithmetic that is itself shown to be right."""
import numpy as np
import pytest

import siggen_cases as cases
import siggen_ref as ref


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: counter / key -> output."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, out in kat:
        assert tuple(int(v) for v in ref.philox4x32_10(np.array(counter, np.uint32), key)) == out
    # vectorised over counters: the same answers row by row
    rows = ref.philox4x32_10(np.array([k[0] for k in kat[:1]] * 3, np.uint32), kat[0][1])
    assert all(tuple(int(v) for v in r) == kat[0][2] for r in rows)


def test_mulhi_and_code_phase_against_python_integers():
    rng = np.random.Generator(np.random.PCG64(3))
    a = rng.integers(0, 1 << 64, 200, dtype=np.uint64)
    b = rng.integers(0, 1 << 64, 200, dtype=np.uint64)
    assert [int(v) for v in ref.mulhi(a, b)] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    sat = dict(code_step_q=ref.q64(1.0 / 4000.0), code_phase0_q=ref.q64(0.7), table_len=1023)
    for t_first in (0, (1 << 32) - 5, (1 << 40) + 12345, (1 << 63) - 3):
        t = np.uint64(t_first) + np.arange(4100, dtype=np.uint64)
        k, f, e = ref.code_phase(sat, t)
        for i in (0, 1, 4, 5, 1199, 1200, 1201, 4099):
            u = sat["code_phase0_q"] + (t_first + i) * sat["code_step_q"]
            assert (int(k[i]), int(f[i]), int(e[i])) == (u >> 64, u & ref.M64, ((u & ref.M64) * 1023) >> 64)
        assert int(e.max()) < 1023


@pytest.mark.parametrize("doppler_hz", [1234.5, -3999.0, 0.0, -1e-9, 4e6, -2.5e6, 562500.0 * -7 + 4e6])
def test_plan_is_floor_of_x_times_two_to_the_64(doppler_hz):
    import gnsscorr
    from fractions import Fraction
    fs = 4e6
    sat = gnsscorr.SiggenSatellite(doppler_hz, 1.023e6 * (1 + doppler_hz / 1575.42e6) / 1023.0 / fs, [dict(table=np.ones(4, np.float32))],
        carrier_phase0_turns=-0.3, code_phase0_periods=0.61)
    words = gnsscorr.siggen_plan(sat, fs)
    assert words == ref.plan_words(doppler_hz, -0.3, 0.61, sat.c.code_periods_per_sample, fs)
    # the rule itself in exact rationals: floor(x 2^64) of the DOUBLE x
    assert words[0] == int(Fraction(sat.c.code_periods_per_sample) * (1 << 64))
    assert words[1] == int(Fraction(0.61) * (1 << 64))
    q = doppler_hz / fs
    x = Fraction(ref.frac(q))
    assert words[2] == int(x * (1 << 64)) and 0 <= words[2] < 1 << 64
    if doppler_hz < 0 and x != 0:
        # a negative frequency is the two's complement of the positive step, to the resolution of a double near 1
        assert abs(((1 << 64) - words[2]) - int(Fraction(-q) * (1 << 64))) <= 1 << 12
    assert words[3] == int(Fraction(ref.frac(-0.3)) * (1 << 64))


@pytest.mark.parametrize("fs", [4_000_000, 6_625_000])
@pytest.mark.parametrize("delay_chips", [0, 600, 1022])
@pytest.mark.parametrize("prn", [1, 10, 32])
def test_l1_ca_sequence_is_the_library_sampled_generator_repeated(prn, delay_chips, fs):
    """Doppler 0 and phase 0: the carrier is exactly 1 and the noise-free stream IS the sampled code, sample for sample."""
    import gnsscorr
    sat, sigma = gnsscorr.siggen_reference_satellite("G", "1C", prn, 44.0, 0.0, delay_chips, 0, fs, noise_flag=False)
    assert sigma == 0.0 and sat.c.amplitude == 1.0 and sat.c.table_len == 1023
    n = fs // 1000
    x = ref.generate([ref.from_satellite(sat, fs)], 0.0, 0, 0, 3 * n + 17)
    sampled = gnsscorr.gps_l1_ca_code_gen_complex_sampled(prn, fs, 1023 - delay_chips)
    assert len(sampled) == n
    assert np.array_equal(x, np.tile(sampled, 4)[:3 * n + 17].astype(np.complex128))


def test_reference_keys_of_the_other_signals():
    import gnsscorr
    fs = 4e6
    glo, sigma = gnsscorr.siggen_reference_satellite("R", "1G", 10, 44.0, 250.0, 100, 0, fs, bw_bb=0.97, intermediate_freq_hz=0.0)
    assert sigma == 1.0 and glo.c.table_len == 511 and glo.c.n_components == 1
    assert glo.c.doppler_hz == 562500.0 * -7 + 250.0
    assert glo.c.amplitude == pytest.approx(np.sqrt(10 ** 4.4 / (0.97 * fs / 2)), rel=1e-12)
    e1, _ = gnsscorr.siggen_reference_satellite("E", "1B", 11, 44.0, 0.0, 0, 0, fs, data_flag=True)
    assert e1.c.table_len == 49104 and e1.c.n_components == 2 and e1.c.code_periods_per_sample == 1.0 / 16000.0
    assert (e1.c.comp[0].gain, e1.c.comp[1].gain, e1.c.comp[0].periods_per_symbol, e1.c.comp[1].secondary_len) == (1.0, -1.0, 1, 25)
    assert e1.c.amplitude == pytest.approx(np.sqrt(10 ** 4.4 / (fs / 2) / 2), rel=1e-12)
    # the noise-free E1-B component at delay 0 is the CBOC table read by the exact ceil((i + 1) L / N) - 1 rule.  (The library's
    # sampled CBOC generator evaluates that quotient in float32, near 49104, and lands one entry off at isolated samples -- 14 of
    # 16000 here -- so it is not the yardstick for this signal.)
    d = ref.from_satellite(e1, fs)
    x = ref.generate([dict(d, amplitude=1.0, comps=[dict(d["comps"][0], periods_per_symbol=0)])], 0.0, 0, 0, 16000)
    i = np.arange(16000)
    assert np.array_equal(x.real, e1.tables[0].astype(np.float64)[-(-(i + 1) * 49104 // 16000) - 1]) and not np.any(x.imag)
    e5, _ = gnsscorr.siggen_reference_satellite("E", "5X", 7, 44.0, 0.0, 0, 3, 32e6, data_flag=True)
    assert e5.c.table_len == 10230 and (e5.c.comp[0].axis, e5.c.comp[1].axis) == (0, 1)
    assert (e5.c.comp[0].secondary_len, e5.c.comp[1].secondary_len, e5.c.comp[0].periods_per_symbol, e5.c.comp[1].period_offset) == (20, 100, 20, 3)
    with pytest.raises(gnsscorr.GnsscorrError, match="unknown system / signal"):
        gnsscorr.siggen_reference_satellite("C", "B1", 1, 44.0, 0.0, 0, 0, fs)


@pytest.fixture(scope="module")
def noise_2_20():
    return ref.noise(5, 0, 1 << 20)


def test_noise_statistics_of_the_restatement(noise_2_20):
    """2^20 samples, sigma 1: five standard deviations of each estimator.  Deterministic for the seed."""
    g = noise_2_20
    n = g.size
    re, im = g.real, g.imag
    for part in (re, im):
        assert abs(part.mean()) <= 5 / np.sqrt(n)
        assert abs(part.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
        assert abs(np.mean(part[1:] * part[:-1])) <= 5 / np.sqrt(n)   # lag-1 autocorrelation
    assert abs(np.mean(re * im)) <= 5 / np.sqrt(n)
    assert np.abs(g).max() <= np.sqrt(-2 * np.log(2.0 ** -24)) + 1e-12  # r <= 5.77


def test_shared_scene_has_the_events_the_parity_test_wants():
    """A symbol change of PRN 7 and a code-period wrap of E1 fall inside the first 11999 samples."""
    import gnsscorr
    sats, _, _ = cases.shared_scene(gnsscorr)
    d = [ref.from_satellite(s, cases.FS) for s in sats]
    t = np.arange(11999, dtype=np.uint64)
    k7 = ref.code_phase(d[1], t)[0]
    assert len(np.unique((k7 + np.uint64(18)) // np.uint64(20))) == 2
    assert len(np.unique(ref.code_phase(d[2], t)[0])) == 2
    assert ref.amplitude_bound(d) == pytest.approx(0.3 + 0.25 + 0.2 * 2 * float(np.max(np.abs(d[2]["comps"][0]["table"]))))


def test_oracle_detects_the_acquisition_scene_on_the_restated_stream(oracle):
    """The conditions test_siggen_gpu.py asserts of the device's search hold for the CPU oracle on the restatement's samples."""
    import gnsscorr
    sats, sigma, seed = cases.acquisition_scene(gnsscorr)
    x = ref.generate([ref.from_satellite(s, cases.FS) for s in sats], sigma, seed, 0, cases.N).astype(np.complex64)
    fs = cases.FS
    results = []
    for prn in range(1, 33):
        # a block per satellite, as in the reference: its magnitude is kept from dwell to dwell
        p = oracle.pcps(fs_in=fs, sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=4000.0, samples_per_chip=4,
            doppler_max=5000, doppler_step=250)
        p.set_local_code(oracle.gps_l1_ca_code_sampled(prn, fs))
        q = p.core(x)
        results.append((float(q.test_statistics), float(q.doppler), float(q.indext)))
    cases.check_acquisition(results)


def test_oracle_meets_the_reference_limits_on_its_first_generator_configuration(oracle):
    """gps_l1_ca_pcps_acquisition_gsoc2013_test.cc, configuration 1: G PRN 10, 44 dB, 750 Hz, 600 chips, no noise, no data, BW_BB
    0.97, 4 Msps; delay error below 0.5 chip, Doppler error below 2 / (3 x 1 ms) Hz."""
    import gnsscorr
    fs = cases.FS
    sat, sigma = gnsscorr.siggen_reference_satellite("G", "1C", 10, 44.0, 750.0, 600, 0, fs, bw_bb=0.97, data_flag=False, noise_flag=False)
    x = ref.generate([ref.from_satellite(sat, fs)], sigma, 0, 0, cases.N).astype(np.complex64)
    p = oracle.pcps(fs_in=fs, sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=4000.0, samples_per_chip=4,
        doppler_max=10000, doppler_step=250)
    p.set_local_code(oracle.gps_l1_ca_code_sampled(10, fs))
    q = p.core(x)
    assert abs(600.0 - q.indext * 1023.0 / 4000.0) < 0.5
    assert abs(750.0 - q.doppler) < 2.0 / (3 * 1e-3)
