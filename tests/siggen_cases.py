"""The scenes the signal generator's tests share (tests/test_siggen_ref.py on the CPU, tests/test_siggen_gpu.py on the device): each
is a list of gnsscorr.SiggenSatellite plus noise sigma and seed, so that the device and the numpy restatement (tests/siggen_ref.py)
are given the same doubles and tables."""
import numpy as np

FS = 4_000_000
N = 4000  # samples per GPS code period at FS
GPS_L1_HZ = 1575.42e6


def gps_satellite(gnsscorr, prn, doppler_hz, amplitude, code_phase0_periods, carrier_phase0_turns=0.0, data=False, period_offset=0,
        code_doppler=True, fs=FS):
    """One BPSK component of 1023 entries; the code rate follows the carrier Doppler when code_doppler."""
    rate = 1.023e6 * (1.0 + (doppler_hz / GPS_L1_HZ if code_doppler else 0.0))
    comp = dict(table=gnsscorr.gps_l1_ca_code_gen_float(prn), periods_per_symbol=20 if data else 0, period_offset=period_offset)
    return gnsscorr.SiggenSatellite(doppler_hz, rate / 1023.0 / fs, [comp], amplitude=amplitude, carrier_phase0_turns=carrier_phase0_turns,
        code_phase0_periods=code_phase0_periods)


def shared_scene(gnsscorr):
    """GPS PRN 1 at +1234.5 Hz with the matching code Doppler, GPS PRN 7 at -3999 Hz with data, Galileo E1 PRN 11 with both
    components and the secondary code; sigma = sqrt(0.5), seed 5.  The offsets put a data-symbol change of PRN 7, a code-period wrap
    of E1 (a new E1-B symbol and a sign change of the E1-C secondary code) inside the first 11999 samples."""
    e1, _ = gnsscorr.siggen_reference_satellite("E", "1B", 11, 45.0, 0.0, 3000, 0, FS, data_flag=True, noise_flag=True)
    e1.c.doppler_hz = 500.25
    e1.c.amplitude = 0.2
    e1.c.carrier_phase0_turns = 0.7
    e1.c.comp[1].period_offset = 1  # CS25 symbols 1 -> 2 are '0' -> '1'
    sats = [gps_satellite(gnsscorr, 1, 1234.5, 0.3, 0.2503, carrier_phase0_turns=0.1),
        gps_satellite(gnsscorr, 7, -3999.0, 0.25, 0.61, carrier_phase0_turns=-0.3, data=True, period_offset=18), e1]
    return sats, float(np.sqrt(0.5)), 5


# ---- source to acquisition: four GPS satellites at 50 dB-Hz in CN(0, 1) noise ----
ACQ_PRNS = [3, 11, 19, 28]
ACQ_DOPPLERS = [-3250.0, -250.0, 1750.0, 4500.0]  # all on the 250 Hz grid
ACQ_DELAYS = [1234.3, 77.6, 3999.2, 2500.5]       # samples from sample 0 to the start of a code period: fractions of a chip
ACQ_SEED = 11


def acquisition_scene(gnsscorr):
    amplitude = float(np.sqrt(10.0 ** (50.0 / 10.0) / FS))
    sats = [gps_satellite(gnsscorr, prn, fd, amplitude, (1.0 - delay / N) % 1.0, carrier_phase0_turns=0.13 * (i + 1), code_doppler=False)
        for i, (prn, fd, delay) in enumerate(zip(ACQ_PRNS, ACQ_DOPPLERS, ACQ_DELAYS))]
    return sats, float(np.sqrt(0.5)), ACQ_SEED


def check_acquisition(results):
    """results: 32 (test statistic, Doppler in Hz, delay in samples), PRN 1 first.  The four present PRNs hold the four highest
    statistics, each with its exact grid Doppler and its delay within one sample (circularly)."""
    stats = np.array([r[0] for r in results])
    top = sorted(int(i) + 1 for i in np.argsort(stats)[-4:])
    assert top == ACQ_PRNS, (top, stats)
    for prn, fd, delay in zip(ACQ_PRNS, ACQ_DOPPLERS, ACQ_DELAYS):
        _, doppler, indext = results[prn - 1]
        assert doppler == fd, (prn, doppler, fd)
        d = abs(indext - delay) % N
        assert min(d, N - d) <= 1.0, (prn, indext, delay)


# ---- source to closed loop: one satellite with data bits and a consistent code Doppler ----
TRK_PRN, TRK_DOPPLER, TRK_DELAY, TRK_CN0, TRK_SEED = 14, 1500.0, 1000.4, 48.0, 21


def tracking_scene(gnsscorr):
    amplitude = float(np.sqrt(10.0 ** (TRK_CN0 / 10.0) / FS))
    return [gps_satellite(gnsscorr, TRK_PRN, TRK_DOPPLER, amplitude, (1.0 - TRK_DELAY / N) % 1.0, carrier_phase0_turns=0.05, data=True)], float(np.sqrt(0.5)), TRK_SEED
