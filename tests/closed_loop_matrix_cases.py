"""The closed-loop matrix's case table (test infrastructure): signals, loop configurations, sample formats and engine shapes shared by
tests/test_closed_loop_matrix_gpu.py (every kernel instantiation on the device) and tests/test_closed_loop_matrix_inputs.py (the same
inputs through the CPU restatement alone).

Shapes: fs = 5.001 MHz and a 1 ms code period, so a period is 5001 samples -- two whole 2048-sample chunks and a ragged one at 1024
threads, ten chunks at 256 -- and, the block length being odd, the window start walks through all eight residues mod 8 samples (every
16-byte phase of float, int16 and int8 loads) within 24 periods.  3 taps: a random +-1 replica of 1023 code samples at 1 per chip;
5 taps: 2046 code samples at 2 per chip; pilot tracking: a second random replica of the same length as the data component."""
import numpy as np

FS = 5.001e6
N = 5001
N_EP = 24
CN0 = 50.0
FC = 1575.42e6
FORMATS = ("f32", "i16", "i8")
SCALE = {"f32": 1.0, "i16": 300.0, "i8": 25.0}
CLIP = {"i16": 32767, "i8": 127}
DTYPE = {"f32": np.float32, "i16": np.int16, "i8": np.int8}
AMP = float(np.sqrt(10 ** (CN0 / 10) / FS))
HD_SMOOTHER = 6

# (taps, pilot, high_dyn) -> (seed, Doppler [Hz], code delay [samples]); "large": 5 taps, pilot, 8000 code samples (4 Mchip/s at 2 per
# chip: about 1.6 code samples per input sample), whose doubled image (129 KiB) is still resident.
# The remainder of the first block length is T_prn's own fraction, N |Doppler| / fc = 3.2e-6 samples per Hz, and it grows by as much
# every period: Dopplers of 1.6 kHz and more keep every block length 4e-3 samples and more from a whole sample
# (test_closed_loop_matrix_inputs.py asserts 1e-3), so that the device and the restatement cannot take different block lengths.
CASES = {
    (3, False, False): (1101, 1680.0, 1234.0),
    (3, False, True): (1102, -2210.0, 777.0),
    (3, True, False): (1103, 2871.0, 3100.0),
    (3, True, True): (1104, -3234.0, 4321.0),
    (5, False, False): (1105, 2345.0, 2222.0),
    (5, False, True): (1106, -3010.0, 150.0),
    (5, True, False): (1107, -1932.0, 4850.0),
    (5, True, True): (1108, 3777.0, 1999.0),
    "large": (1109, 1850.0, 3456.0),
    # the large row with the high-dynamics kernels: only ever a slot of the all-high-dynamics mixed engine on the window image
    "large_hd": (1109, 1850.0, 3456.0),
}
MATRIX = [k for k in CASES if isinstance(k, tuple)]
REFERENCED = MATRIX + ["large"]  # the configurations that are run through the restatement


def shape(key):
    """(taps, pilot, high_dyn, code samples, code samples per chip) of a case."""
    if key == "large":
        return 5, True, False, 8000, 2
    if key == "large_hd":
        return 5, True, True, 8000, 2
    taps, pilot, hd = key
    return taps, pilot, hd, (1023 if taps == 3 else 2046), (1 if taps == 3 else 2)


_built = {}


def build(key):
    """The case's signal and configuration: dict(code, data_code or None, conf, sync or None, x complex64)."""
    if key in _built:
        return _built[key]
    from test_loop_sync_gpu import _stream
    taps, pilot, hd, L, spc = shape(key)
    seed, doppler, delay = CASES[key]
    rng = np.random.Generator(np.random.PCG64(seed))
    code = (rng.integers(0, 2, L) * 2 - 1).astype(np.float32)
    data_code = (rng.integers(0, 2, L) * 2 - 1).astype(np.float32) if pilot else None
    comps = [(code, [1.0], 1.0)]
    if pilot:
        comps.append((data_code, rng.integers(0, 2, 97) * 2.0 - 1.0, 1.0))
    x = _stream(comps, FS, N * (N_EP + 3), doppler, delay, CN0, seed + 50, L * 1000.0)
    conf = dict(fs_in=FS, signal_carrier_freq_hz=FC, code_chip_rate_hz=L * 1000.0 / spc, code_period_s=0.001, carrier_lock_th=0.85,
        code_length_chips=L // spc, code_samples_per_chip=spc, vector_length=N, pull_in_time_s=0, veml=int(taps == 5), pll_filter_order=3,
        dll_filter_order=2, enable_fll_pull_in=0, enable_fll_steady_state=0, cn0_samples=10, cn0_min=25, max_lock_fail=50, pll_bw_hz=35.0,
        dll_bw_hz=2.0, fll_bw_hz=10.0, early_late_space_chips=(0.15 if taps == 5 else 0.5), very_early_late_space_chips=(0.6 if taps == 5 else 0.0),
        acq_samplestamp_samples=0, sample_counter=0, acq_delay_samples=delay, acq_doppler_hz=doppler + 3.0,
        high_dyn_smoother_length=(HD_SMOOTHER if hd else 0))
    sync = dict(extend_correlation_symbols=1, track_pilot=True, symbols_per_bit=1) if pilot else None
    _built[key] = dict(code=code, data_code=data_code, conf=conf, sync=sync, x=x)
    return _built[key]


_samples = {}


def samples(key, fmt):
    """(what the device reads: an (n, 2) array of the format's type; the same samples as complex64 for the restatement and the float
    anchor).  The stream is quantised once per format: round(x * scale), clipped."""
    if (key, fmt) not in _samples:
        x = build(key)["x"]
        if fmt == "f32":
            _samples[key, fmt] = (x.view(np.float32).reshape(-1, 2), x)
        else:
            q = np.clip(np.round(x.view(np.float32).reshape(-1, 2) * np.float32(SCALE[fmt])), -CLIP[fmt], CLIP[fmt]).astype(DTYPE[fmt])
            f = np.ascontiguousarray(q.astype(np.float32))
            _samples[key, fmt] = (q, f.view(np.complex64).reshape(-1))
    return _samples[key, fmt]


_refs = {}


def reference(oracle, key, fmt):
    """The CPU restatement's records for the case on the format's samples cast to float; computed once, never modified."""
    if (key, fmt) not in _refs:
        from closed_loop_ref import run
        c = build(key)
        _refs[key, fmt] = run(oracle, samples(key, fmt)[1], c["code"], c["conf"], N_EP, sync=c["sync"], data_code=c["data_code"])
    return _refs[key, fmt]


# ---- engine shapes: how each LDS code-image mode is reached, and the launch plan's argument tuple (tests/loop_plan_selftest.cpp) ----
MIXED_KINDS = [(3, False), (5, False), (3, True), (5, True)]


def engine_shape(mode, key, n_cus):
    """(channels, max_code_len, resident) of the plain engine that runs `key` in `mode`."""
    L = shape(key)[3]
    if mode == "resident":
        return 1, L, 1
    if mode == "window_pilot":  # (2 * 12000 + 64) * 2 floats is over the 150 KiB rule
        return 1, 12000, 0
    if mode == "window_data":  # more slots than CUs and an image over 64 KiB; only slot 0 is started
        return n_cus + 1, 8100, 0
    raise ValueError(mode)


def plan_tuple(mode, key, threads, n_cus):
    """`channels,cus,high_dyn,forced_threads,mixed,max_code_len,pilot` of a plain engine; threads = 0 for the high-dynamics kernels."""
    _, pilot, hd, _, _ = shape(key)
    channels, max_len, _ = engine_shape(mode, key, n_cus)
    return "%d,%d,%d,%d,0,%d,%d" % (channels, n_cus, int(hd), threads, max_len, int(pilot))


def mixed_keys(hd, image):
    """The cases in the slots of a mixed engine: 3 / 5 taps x data / pilot, and on the window image the large pilot row, whose started
    8000-sample pilot slot in an engine of more slots than CUs is what takes a mixed engine off the resident image (a mixed engine's
    image follows its started channels, not max_code_len)."""
    keys = [(taps, pilot, hd) for taps, pilot in MIXED_KINDS]
    if image == "window":
        keys.append("large_hd" if hd else "large")
    return keys


def mixed_shape(image, n_cus):
    """(channels, max_code_len, resident) of the mixed engine."""
    return (4, 2046, 1) if image == "resident" else (n_cus + 1, 12000, 0)


def mixed_plan_tuple(hd, image, threads, n_cus):
    channels, max_len, _ = mixed_shape(image, n_cus)
    slots = ",".join("%d/%d/1" % (shape(k)[3], int(shape(k)[1])) for k in mixed_keys(hd, image))
    return "%d,%d,%d,%d,1,%d,0,%s" % (channels, n_cus, int(hd), threads, max_len, slots)


def modes_of(key):
    """The LDS modes a case runs in: resident, and the window mode of its kind."""
    if not isinstance(key, tuple):
        return ["resident"]
    return ["resident", "window_pilot" if key[1] else "window_data"]


def thread_counts(key):
    """Forced workgroup sizes of a case: the high-dynamics kernels always run 256 (0: nothing forced)."""
    return [0] if shape(key)[2] else [1024, 512, 256]


def all_plan_tuples(n_cus):
    """Every (argument tuple, (threads, resident)) the matrix launches with."""
    out = {}
    for key in CASES:
        for mode in modes_of(key):
            for th in thread_counts(key):
                out[plan_tuple(mode, key, th, n_cus)] = (th or 256, engine_shape(mode, key, n_cus)[2])
    for hd in (False, True):
        for image in ("resident", "window"):
            for th in ([0] if hd else [1024, 512, 256]):
                out[mixed_plan_tuple(hd, image, th, n_cus)] = (th or 256, mixed_shape(image, n_cus)[2])
    return out
