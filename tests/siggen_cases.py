"""The scenes the signal generator's tests share (tests/test_siggen_ref.py and tests/test_siggen_matrix_inputs.py on the CPU,
tests/test_siggen_gpu.py and tests/test_siggen_matrix_gpu.py on the device): each is a list of gnsscorr.SiggenSatellite plus noise
sigma and seed, so that the device and the numpy restatement (tests/siggen_ref.py) are given the same doubles and tables."""
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


# ---- the matrix: every signal kind, both axes, every table size and placement, 32 satellites, periods shorter than a run ----
# (tests/test_siggen_matrix_inputs.py holds each scene to the events named here on the restatement alone;
# tests/test_siggen_matrix_gpu.py runs them on the device).  Every number below is written down, none is searched for at test time:
#   w   the first sample of a new code period, set through code_phase0_periods = 1 - (w - 1/2) step.  Every w is no multiple of 4
#       (the wrap falls INSIDE a thread's four consecutive float samples) nor of 1024 (inside a tile, so between the samples i and
#       i + 256 of one thread of the integer kernels).
#   m   the data-symbol block: period_offset = pps m + pps - 1, so that the symbol number goes m -> m + 1 at the first wrap; m is
#       the first block at which the two symbols of that (seed, satellite index, component) differ.
MATRIX_N = 2 * 1024 + 453   # two whole tiles and a ragged one; odd, so that a second call starts at an odd ring position
E5A_N = 33 * 1024 + 453     # E5a's 32000-sample period needs two wraps (see e5a below): the second lies in the last 1537 samples
LDS_FLOATS = 15360          # GC_SIGGEN_LDS_FLOATS of siggen_kernels.h
SAMPLE_NUMBER_EDGES = (2 ** 32 - 700, 2 ** 63 - 513, 2 ** 64 - 600)  # the starts tests/siggen_phase_selftest.cpp uses
EDGE_N = 1500               # the crossings at samples 700, 513 and 600: inside the first tile and, counted from 1, the second
GLONASS_SLOTS = (1, 2, 3, 4, 9, 10, 11, 12)  # frequency channels 1, -4, 5, 6, -2, -7, 0, -1
Q_ONLY_TABLE = (0.5, -1.25, 0.75, 1.5, -0.625, -2.0, 1.125)
SEC3 = (1, -1, 1)
SEC5 = (1, 1, -1, 1, -1)


def place_wrap(sat, w):
    """Puts the first sample of the satellite's second code period at sample w."""
    sat.c.code_phase0_periods = 1.0 - (w - 0.5) * sat.c.code_periods_per_sample
    return sat


def _set(sat, doppler_hz, amplitude, carrier_phase0_turns, w, offsets):
    sat.c.doppler_hz, sat.c.amplitude, sat.c.carrier_phase0_turns = doppler_hz, amplitude, carrier_phase0_turns
    for c, off in enumerate(offsets):
        sat.c.comp[c].period_offset = off
    return place_wrap(sat, w)


def _sec100():
    return np.where(np.random.Generator(np.random.PCG64(100)).integers(0, 2, 100) == 1, -1, 1).astype(np.int8)


def matrix_gps(gnsscorr, fs=FS, prn=5, doppler_hz=2345.5, amplitude=0.3, phase=0.15, w=1201, m=0):
    """GPS L1 C/A with data: symbol m -> m + 1 at sample w."""
    sat = gps_satellite(gnsscorr, prn, doppler_hz, amplitude, 0.0, carrier_phase0_turns=phase, data=True, period_offset=20 * m + 19, fs=fs)
    return place_wrap(sat, w)


def matrix_glonass(gnsscorr, fs=FS, slot=10, doppler_hz=250.0, amplitude=0.25, phase=-0.2, w=1703, m=0):
    """GLONASS L1 from the reference constructor (intermediate frequency 0: the carrier is the FDMA offset plus the Doppler),
    with data."""
    sat, _ = gnsscorr.siggen_reference_satellite("R", "1G", slot, 45.0, doppler_hz, 100, 0, fs, data_flag=True, intermediate_freq_hz=0.0)
    return _set(sat, sat.c.doppler_hz, amplitude, phase, w, [20 * m + 19])


def matrix_e1(gnsscorr, fs=FS, prn=11, doppler_hz=-1500.75, amplitude=0.25, phase=0.7, w=1301, m=0, pilot_offset=1):
    """Galileo E1 B + C from the reference constructor; CS25 symbols 1 -> 2 are '0' -> '1', so pilot_offset = 1 changes the
    secondary code's sign at w."""
    sat, _ = gnsscorr.siggen_reference_satellite("E", "1B", prn, 45.0, 0.0, 3000, 0, fs, data_flag=True)
    return _set(sat, doppler_hz, amplitude, phase, w, [m, pilot_offset])


def matrix_e5a(gnsscorr, fs=32e6, prn=7, doppler_hz=3210.5, amplitude=0.3, phase=0.35, w=901, i_offset=19, q_offset=0):
    """Galileo E5a I + Q from the reference constructor.  The I component's 20 periods per symbol run in step with its secondary
    code of 20, and CS20 ends and begins with '1': a symbol change (i_offset = 20 m + 19) never coincides with a sign change of
    the secondary code; the boundary after it (CS20 symbols 0 -> 1 are '1' -> '0') has one."""
    sat, _ = gnsscorr.siggen_reference_satellite("E", "5X", prn, 45.0, 0.0, 0, 0, fs, data_flag=True)
    return _set(sat, doppler_hz, amplitude, phase, w, [i_offset, q_offset])


def matrix_q_only(gnsscorr, fs=FS, amplitude=0.2):
    """One component on the imaginary axis, 7 entries that are not +-1, negative gain, a period of 700.3 samples."""
    comp = dict(table=np.array(Q_ONLY_TABLE, np.float32), axis=1, gain=-0.75)
    return place_wrap(gnsscorr.SiggenSatellite(-777.25, 1.0 / 700.3, [comp], amplitude=amplitude, carrier_phase0_turns=0.45), 333)


def matrix_two_axes_small(gnsscorr, fs=FS, amplitude=0.3, m=0, offset0=0):
    """The reverse of E5a, small enough for LDS: 2 x 4092 entries of +-1 on axes (1, 0), secondary codes of 3 and 100, data of 2
    periods per symbol on the second component; a period of 1000.7 samples: wraps at 411, 1412 and 2413."""
    rng = np.random.Generator(np.random.PCG64(4092))
    tables = np.where(rng.integers(0, 2, (2, 4092)) == 1, -1.0, 1.0).astype(np.float32)
    comps = [dict(table=tables[0], axis=1, secondary=np.array(SEC3, np.int8), period_offset=offset0),
        dict(table=tables[1], axis=0, secondary=_sec100(), periods_per_symbol=2, period_offset=2 * m + 1, gain=0.5)]
    return place_wrap(gnsscorr.SiggenSatellite(1999.5, 1.0 / 1000.7, comps, amplitude=amplitude, carrier_phase0_turns=-0.1), 411)


def matrix_short_period(gnsscorr, fs=FS, period=3.7):
    """A code period of 3.7 samples: a period boundary inside nearly every run of four consecutive samples, at every place of it,
    and 69 whole periods from a thread's sample i to its sample i + 256.  Four consecutive samples span 3 / 3.7 of a period, so
    never two boundaries: the row very_short_period, 1.37 samples, has two or three in every run (and 186 periods in 256
    samples).  Data of one period per symbol on the real axis, a secondary code of 5 on the imaginary."""
    comps = [dict(table=np.array([1.0, -0.5], np.float32), axis=0, periods_per_symbol=1, period_offset=3),
        dict(table=np.array([-0.75, 1.0], np.float32), axis=1, secondary=np.array(SEC5, np.int8), period_offset=1)]
    return gnsscorr.SiggenSatellite(-1234.5, 1.0 / period, comps, amplitude=0.3, carrier_phase0_turns=0.6, code_phase0_periods=0.3)


def matrix_long_period(gnsscorr, fs=FS):
    """49104 entries, and the 2501 samples are 0.6 of one code period: the period never wraps, every sample reads another entry."""
    table = np.random.Generator(np.random.PCG64(49104)).uniform(0.5, 1.5, 49104) * np.where(np.arange(49104) % 3 == 0, -1.0, 1.0)
    comp = dict(table=table.astype(np.float32), periods_per_symbol=1, period_offset=5)
    return gnsscorr.SiggenSatellite(4321.0, 0.6 / MATRIX_N, [comp], amplitude=0.3, carrier_phase0_turns=0.25, code_phase0_periods=0.31)


def matrix_mix32(gnsscorr):
    """8 each of GPS, GLONASS (distinct channels), E1 and E5a at 32 Msps: 8 x (1023 + 511 + 2 x 49104 + 2 x 10230) table entries.
    Satellite s has amplitude 0.05 + 0.15 s / 31, its wrap at sample 301 + 67 s (+ 1 where that is a multiple of 4) and its own
    Doppler and phase.  An E5a I component cannot have both events in 2501 samples (matrix_e5a): the even ones change the data
    symbol, the odd ones the secondary code's sign."""
    fs = 32e6
    sats = []
    for s in range(32):
        w = 301 + 67 * s
        w += 1 if w % 4 == 0 else 0
        common = dict(fs=fs, doppler_hz=-4000.0 + 258.5 * s, amplitude=0.05 + 0.15 * s / 31.0, phase=0.03 * s, w=w)
        kind, i = divmod(s, 8)
        if kind == 0:
            sats.append(matrix_gps(gnsscorr, prn=1 + 3 * i, m=MIX32_BLOCKS[s], **common))
        elif kind == 1:
            sats.append(matrix_glonass(gnsscorr, slot=GLONASS_SLOTS[i], m=MIX32_BLOCKS[s], **common))
        elif kind == 2:
            sats.append(matrix_e1(gnsscorr, prn=2 + 4 * i, m=MIX32_BLOCKS[s], pilot_offset=1, **common))
        else:
            sats.append(matrix_e5a(gnsscorr, prn=3 + 4 * i, i_offset=20 * MIX32_BLOCKS[s] + 19 if i % 2 == 0 else 0, q_offset=MIX32_Q_OFFSETS[i], **common))
    return sats


# the first symbol block m at which symbols m and m + 1 of (seed, satellite index, component) differ; for the E5a Q components, a
# period_offset at which the PRN's secondary code of 100 changes sign
SEEDS = dict(gps=3, glonass=4, e1=5, e5a=6, q_only=7, two_axes_small=8, short_period=9, very_short_period=11, long_period=10, mix32=32, mix_lds=15)
BLOCKS = dict(gps=0, glonass=0, e1=1, e5a=0, two_axes_small=0)
E5A_Q_OFFSET = 0
MIX32_BLOCKS = (0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 2, 0, 0, 5, 2, 0, 0, 0, 0, 0, 5, 1, 1)
MIX32_Q_OFFSETS = (0, 0, 2, 2, 0, 1, 1, 2)
MIX_LDS_BLOCKS = (2, 1, 2)  # gps, glonass, two_axes_small as satellites 0, 1, 2


# (GC_IQ_I16, GC_IQ_I8) output scales: full scale near the 88th percentile of the restated components' magnitudes, so that some
# components clip and fewer than a quarter do (tests/test_siggen_matrix_inputs.py asserts it of the restated quantisation)
SCALES = dict(gps=(110000.0, 430.0), glonass=(135000.0, 524.0), e1=(75000.0, 290.0), e5a=(79000.0, 305.0), q_only=(160000.0, 610.0),
    two_axes_small=(99000.0, 390.0), short_period=(94000.0, 360.0), very_short_period=(94000.0, 360.0), long_period=(98000.0, 380.0), mix32=(24000.0, 95.0), mix_lds=(46000.0, 180.0))


def matrix_mix_lds(gnsscorr):
    """gps + glonass + two_axes_small + q_only at 4 Msps: 1023 + 511 + 8184 + 7 table entries, under LDS_FLOATS."""
    return [matrix_gps(gnsscorr, m=MIX_LDS_BLOCKS[0]), matrix_glonass(gnsscorr, m=MIX_LDS_BLOCKS[1]),
        matrix_two_axes_small(gnsscorr, m=MIX_LDS_BLOCKS[2]), matrix_q_only(gnsscorr)]


# name -> (sats(gnsscorr), sigma, fs, n); the seed is SEEDS[name] and every scene starts at t0 = 0
MATRIX = {
    "gps": (lambda g: [matrix_gps(g, m=BLOCKS["gps"])], 0.0, FS, MATRIX_N),
    "glonass": (lambda g: [matrix_glonass(g, m=BLOCKS["glonass"])], 0.0, FS, MATRIX_N),
    "e1": (lambda g: [matrix_e1(g, m=BLOCKS["e1"])], 0.0, FS, MATRIX_N),
    "e5a": (lambda g: [matrix_e5a(g, i_offset=20 * BLOCKS["e5a"] + 19, q_offset=E5A_Q_OFFSET)], 0.0, 32e6, E5A_N),
    "q_only": (lambda g: [matrix_q_only(g)], 0.0, FS, MATRIX_N),
    "two_axes_small": (lambda g: [matrix_two_axes_small(g, m=BLOCKS["two_axes_small"])], 0.0, FS, MATRIX_N),
    "short_period": (lambda g: [matrix_short_period(g)], 0.0, FS, MATRIX_N),
    "very_short_period": (lambda g: [matrix_short_period(g, period=1.37)], 0.0, FS, MATRIX_N),
    "long_period": (lambda g: [matrix_long_period(g)], 0.0, FS, MATRIX_N),
    "mix32": (matrix_mix32, 0.5, 32e6, MATRIX_N),
    "mix_lds": (matrix_mix_lds, 0.25, FS, MATRIX_N),
}
SINGLE = tuple(name for name in MATRIX if not name.startswith("mix"))


def matrix_scene(gnsscorr, name):
    """(sats, sigma, seed, fs, n, t0) of a row of MATRIX, freshly built: the caller may change its satellites."""
    build, sigma, fs, n = MATRIX[name]
    return build(gnsscorr), sigma, SEEDS[name], fs, n, 0


def scene_dict(gnsscorr, name, sats=None, **changes):
    """The row as the dict the device tests pass around: sats, sigma, seed, fs, n, t0 and dicts, the restatement's satellites."""
    import siggen_ref as ref
    built, sigma, seed, fs, n, t0 = matrix_scene(gnsscorr, name)
    sats = built if sats is None else sats
    d = dict(name=name, sats=sats, sigma=sigma, seed=seed, fs=fs, n=n, t0=t0)
    d.update(changes)
    d["dicts"] = [ref.from_satellite(s, d["fs"]) for s in sats]
    return d


def exact_variant(sats):
    """The same codes, symbols and axes under a carrier that is exactly 1: Doppler 0 (for GLONASS the FDMA offset too), carrier
    phase 0, amplitude 1.  The code phase words are untouched."""
    for sat in sats:
        sat.c.doppler_hz, sat.c.carrier_phase0_turns, sat.c.amplitude = 0.0, 0.0, 1.0
    return sats
