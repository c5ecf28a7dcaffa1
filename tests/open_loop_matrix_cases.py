"""The open-loop matrix's case table (test infrastructure, free of GPU calls): one launch per reachable instantiation of
trk_multicorrelator_kernel -- tap counts 1..8 x (plain, high-dynamics, complex chips) x (F32, I16, I8) and the 16-bit mode through
TrackingBatch, the high-dynamics resampler through the level-1 object -- shared by tests/test_open_loop_matrix_gpu.py (the launches on
the device against tests/open_loop_ref.py) and tests/test_open_loop_matrix_inputs.py (the same inputs on the CPU: the restatement
against the compiled oracle, the size of the bar against one sample, and the path of trk_epoch / trk_loop every window takes).

Streams: fs = 4 MHz, two GPS C/A satellites at 45 dB-Hz in unit-variance noise, quantised once per format (round(x * scale), clipped;
the 16-bit mode at test_16sc_gpu.py's scale of 16, so that no sum leaves the int16 range).  In the matrix stream every sample outside
every window is poison: NaN / Inf for F32, full scale for I16 / I8.

The matrix launch: 2 channels x 11 epochs, GPS C/A chips.  Channel 1 is bound 5 samples past the (16-sample aligned) allocation, so the
address of its window at sample_offset 0 is 5 past a boundary the channel's buffer does not reach back to (the ragged head is loaded
sample by sample), and its last window ends with the buffer (so is the ragged tail).  Every record has its own carrier phase and step,
code phase and step, near the satellite's true ones.  WINDOWS lists the windows and the branch of trk_loop each is there for;
test_open_loop_matrix_inputs.py asserts each is taken.  Every launch runs with 1 and with 3 slices.

High-dynamics modes: the taps are tap 0 delayed by whole samples and wrapped at N, and the reference needs the delays below N (it
memcpy()s N - delay floats), so their windows of 1 and 2 samples are 64 samples longer, as in test_fuzz_gpu.py.  The high-dynamics
resampler with the plain rotator (TRK_MODE_HD_RESAMPLER) is reached through the level-1 object's 6-argument overload alone, whose
input is float: TRK_FORMAT_TRAITS (trk_batch_plan.h) gives that mode the F32 format only, trk_launch compiles no other kernel for it, and
LEVEL1_ONLY below says how the matrix reaches it.

Smaller tables: RESYNC (a window of 66 chunks and 77 samples, carrier step 1.3 rad per sample: the exact re-evaluation of the rotators
every 64 chunks), TABLE PATHS (L = 8184, or 7936 complex chips, N = 4608, 2 slices, records on the device: the launch's LDS is below the table, one record
fits its window, two read the table from global memory), TINY CODE (L = 31, a window that wraps the code more than twice: the `% L`
fill loop) and LEVEL 1 (the three drop-in objects, every overload, from an odd sample of an aligned array).

Worst |oracle - restatement| / bar per (mode, format) over every record of every table (CPU, test_open_loop_matrix_inputs.py; the
reference's float32 rotator and its drifting modulus against plain maths):
  plain 0.044 / 0.046 / 0.049 (F32 / I16 / I8), complex chips 0.041 / 0.045 / 0.044, high-dynamics 0.372 / 0.372 / 0.373 and
  high-dynamics resampler (level 1, F32; the oracle runs it with the high-dynamics rotator) 0.335: the modulus of the reference's
  phase_doppler drifts as |phase_inc|^n, which the kernel reproduces on purpose and plain maths does not.
Worst |device - restatement| / bar per (mode, format), MI355X (test_open_loop_matrix_gpu.py; 16-bit mode: worst LSB difference):
  plain 0.007 / 0.010 / 0.008 (the resync window; the matrix launch alone: 0.003 / 0.002 / 0.002), complex chips 0.010 / 0.011 / 0.011
  (matrix alone: 0.002), high-dynamics 0.391 / 0.391 / 0.389 (the reference's drift again), high-dynamics resampler 0.001;
  16-bit mode 1 LSB (matrix launch: 0).
Information for whoever changes the loop next, not gates."""
import collections
import os
import subprocess

import numpy as np

from helpers import synth_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FS = 4.0e6
CN0 = 45.0
CHIP_RATE = 1.023e6
FORMATS = ("f32", "i16", "i8")
FORMAT_BIT = {"f32": 1, "i16": 2, "i8": 4}  # 1 << gc_iq_format
SCALE = {"f32": 1.0, "i16": 300.0, "i8": 25.0, "sc16": 16.0}
DTYPE = {"f32": np.float32, "i16": np.int16, "i8": np.int8, "sc16": np.int16}
CLIP = {"i16": 32767, "i8": 127, "sc16": 32767}
MODES = ("plain", "hd_resampler", "hd_full", "complex", "sc16")  # TRK_MODE_* order
HD = ("hd_resampler", "hd_full")
LEVEL1_ONLY = {"hd_resampler": ("f32",)}  # no batch arithmetic selects it; a level-1 call's input is complex float
# the project's bar (tests/test_fuzz_gpu.py): 1e-4 max_t |ref[t]| + NOISE * scale * sqrt(n); exact zeros for n = 0
REL = 1e-4
NOISE = {"plain": 3e-5, "hd_resampler": 3e-5, "hd_full": 3e-5, "complex": 6e-5}
CHUNK = 512  # TRK_CHUNK
ALIGN = 16  # samples: 2 * TRK_ALIGN_PAIRS (level-1 calls: 2)
LDS_MARGIN = 64  # TRK_LDS_MARGIN_FLOATS

BATCH = [(m, f) for m in ("plain", "hd_full", "complex") for f in FORMATS] + [("sc16", "i16")]
TAPS = tuple(range(1, 9))
PRNS = (5, 17)
BIND = (0, 5)  # samples between the allocation's base and the channel's pointer
SLICINGS = (1, 3)

# (channel, N, address of the first sample mod 16, tag).  The order is the order in memory; a channel's epochs are its rows in order.
WINDOWS = [
    (1, 2597, 5, "first"),    # sample_offset 0 behind an unaligned pointer: lc0 == 1, the head goes through load_masked
    (0, 0, 3, "empty"),       # one all-masked chunk
    (0, 1, 7, "tiny"),
    (1, 2, 10, "tiny"),
    (0, 511, 0, "edge"),      # chunk-boundary lengths at each alignment
    (1, 511, 1, "edge"),
    (0, 512, 1, "edge"),
    (1, 512, 0, "edge"),
    (0, 513, 15, "edge"),
    (1, 513, 1, "edge"),
    (0, 511, 15, "edge"),
    (1, 0, 1, "empty"),
    (0, 513, 0, "edge"),
    (0, 512, 15, "edge"),
    (1, 2048, 0, "aligned"),  # no ragged chunk at all
    (0, 2100, 5, "odd"),      # ragged head, three full chunks (a pair through the two-buffer queue and its odd leftover), ragged tail
    (1, 1, 12, "tiny"),
    (0, 2597, 9, "ragged"),   # ragged head, four full chunks (two pairs), ragged tail; 3 slices: 2 + 2 + 2 chunks
    (1, 2597, 11, "ragged"),
    (0, 2597, 13, "fast"),    # code step ~0.5 chip per sample: one slice spans more chips than the LDS holds
    (1, 2597, 3, "fast"),
    (1, 2597, 7, "last"),     # ends with the channel's buffer: the tail goes through load_masked
]
# (n_chunks, full chunks) of the "edge" windows, worked out by hand: V = N + a samples counted from the boundary, chunk c is full when
# (c > 0 or a == 0) and (c + 1) * 512 <= V
EDGE_CHUNKS = {(511, 0): (1, 0), (512, 0): (1, 1), (513, 0): (2, 1), (511, 1): (1, 0), (512, 1): (2, 0), (513, 1): (2, 0),
    (511, 15): (2, 0), (512, 15): (2, 0), (513, 15): (2, 0)}
GAP = 24  # poison between windows: more than the 15 samples a whole-chunk fetch reaches back

Rec = collections.namedtuple("Rec", "offset n tag args params")  # args: the reference's float32 scalars; params: gnsscorr.EpochParams
Launch = collections.namedtuple("Launch", "table mode fmt n_taps code_len max_code_len codes shifts stream binds n_iq recs slicings on_device")


def shifts_of(n_taps):
    return (np.linspace(-0.7, 0.7, n_taps) if n_taps > 1 else np.zeros(1)).astype(np.float32)


def n_of(n, tag, mode):
    """Window length of a row in `mode`: the high-dynamics resamplers' tiny windows are 64 samples longer."""
    return n + 64 if (mode in HD and tag == "tiny") else n


def _layout():
    starts, pos = [], 0
    for i, (ch, n, res, tag) in enumerate(WINDOWS):
        start = BIND[ch] if i == 0 else pos + GAP + (res - (pos + GAP)) % ALIGN
        assert start % ALIGN == res and start >= BIND[ch]
        starts.append(start)
        pos = start + n_of(n, tag, "hd_full")
    return starts, pos


STARTS, N_MATRIX = _layout()
N_IQ = tuple(N_MATRIX - b for b in BIND)
RESYNC_N = 66 * CHUNK + 77
N_CLEAN = RESYNC_N + 3

# ---- the kernel's reachable instantiations, from the headers (tests/trk_batch_plan_selftest.cpp, built with -DTRK_SELFTEST_TRAITS) ----


def build_selftest(directory):
    exe = os.path.join(str(directory), "trk_batch_plan_selftest")
    csrc = os.path.join(ROOT, "gnss-sdr-1_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Wextra", "-DTRK_SELFTEST_TRAITS", "-D__HIP_PLATFORM_AMD__", "-I", csrc,
        "-I", os.path.join(ROOT, "include"), "-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
        os.path.join(ROOT, "tests", "trk_batch_plan_selftest.cpp"), "-o", exe])
    return exe


def reachable(exe):
    """{(n_taps, mode, fmt)} a caller can reach: GC_MAX_TAPS tap counts x the sample formats TRK_FORMAT_TRAITS gives each mode (the
    ones trk_launch compiles a kernel for), of which a mode of LEVEL1_ONLY can take its listed ones."""
    out = subprocess.run([exe, "traits"], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert out[0].split()[0] == "max_taps" and len(out) == 1 + len(MODES), out
    keys = set()
    for line in out[1:]:
        mode, formats = int(line.split()[0]), int(line.split()[1])
        for fmt in LEVEL1_ONLY.get(MODES[mode], FORMATS):
            if formats & FORMAT_BIT[fmt]:
                keys |= {(t, MODES[mode], fmt) for t in range(1, int(out[0].split()[1]) + 1)}
    return keys


def matrix_keys():
    """{(n_taps, mode, fmt)} the matrix launches."""
    return {(t, m, f) for m, f in BATCH for t in TAPS} | {(t, m, f) for m, fs in LEVEL1_ONLY.items() for f in fs for t in TAPS}


def plan(exe, launch, n_slices, n_cus=256):
    """(n_slices, lds_floats) the host gives the launch (trk_batch_plan.h)."""
    words = 2 if launch.mode == "complex" else 1
    max_len = max(r.n for ch in launch.recs for r in ch)
    max_step = 0.0 if launch.on_device else max(abs(float(r.params.code_phase_step_chips)) + abs(float(r.params.code_phase_rate_step_chips)) * r.n
        for ch in launch.recs for r in ch if r.n > 0)
    arg = "%d,1,%d,%d,%d,1,%d,%.9g,%d/%dx%d,%s" % (n_slices, len(launch.recs[0]), n_cus, MODES.index(launch.mode), max_len, max_step,
        words * (launch.max_code_len + LDS_MARGIN), len(launch.recs), launch.code_len, ",".join("%.9g" % s for s in launch.shifts))
    out = subprocess.run([exe, arg], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return int(out[0]), int(out[1])


# ---- streams ----
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def ca_code(oracle, prn):
    return _once(("ca", prn), lambda: oracle.gps_l1_ca_code(prn).astype(np.float32))


def _float_stream(oracle, name):
    n, seed = (N_MATRIX, 20261) if name == "matrix" else (N_CLEAN, 20262)
    return _once(("x", name), lambda: synth_stream([ca_code(oracle, p) for p in PRNS], int(FS), n, seed=seed, cn0_db_hz=(CN0, CN0), chip_rate=CHIP_RATE))


def _inside(hd):
    mask = np.zeros(N_MATRIX, bool)
    for start, (ch, n, res, tag) in zip(STARTS, WINDOWS):
        mask[start:start + n_of(n, tag, "hd_full" if hd else "plain")] = True
    return mask


def samples(oracle, stream, fmt, hd=False):
    """(what the device reads: an (n, 2) array of the format's type, the matrix stream poisoned outside the windows; the clean
    samples as complex64 -- integers cast to float -- for the references).  fmt "sc16": int16 at the 16-bit mode's scale."""
    def make():
        x = _float_stream(oracle, stream)[0]
        if fmt == "f32":
            q, clean = x.view(np.float32).reshape(-1, 2).copy(), x
        else:
            q = np.clip(np.round(x.view(np.float32).reshape(-1, 2) * np.float32(SCALE[fmt])), -CLIP[fmt], CLIP[fmt]).astype(DTYPE[fmt])
            clean = np.ascontiguousarray(q.astype(np.float32)).view(np.complex64).reshape(-1)
        if stream == "matrix":
            out = ~_inside(hd)
            if fmt == "f32":
                poison = np.array([[np.nan, np.inf], [-np.inf, np.nan], [np.nan, np.nan]], np.float32)
                q[out] = poison[np.arange(out.sum()) % 3]
            else:
                q[out] = [CLIP[fmt], -CLIP[fmt]]
        return q, clean
    return _once(("q", stream, fmt, hd and stream == "matrix"), make)


# ---- records ----
def _f32(v):
    return float(np.float32(v))


def _rec(offset, n, tag, rem_carr, pstep, rem_code, cstep, prate=0.0, crate=0.0):
    import gnsscorr  # gc_epoch_params_fill: a host function
    args = dict(rem_carr=_f32(rem_carr), pstep=_f32(pstep), prate=_f32(prate), rem_code=_f32(rem_code), cstep=_f32(cstep), crate=_f32(crate))
    params = gnsscorr.epoch_params(offset, args["rem_carr"], args["pstep"], args["rem_code"], args["cstep"], n,
        carr_phase_rate_step_rad=args["prate"], code_phase_rate_step_chips=args["crate"])
    return Rec(offset, n, tag, args, params)


def _near_truth(truth, start, rng, L=1023):
    """(rem_carr, pstep, rem_code, cstep) of a window at absolute sample `start`, a little off the satellite's true values."""
    step = truth["code_rate"] / FS
    rem = -((truth["tau0"] + start * step) % L)
    rem = rem + L if rem < -L / 2 else rem
    return ((truth["phi"] + 2 * np.pi * truth["doppler"] * start / FS) % (2 * np.pi) + rng.uniform(-3, 3), 2 * np.pi * truth["doppler"] / FS + rng.uniform(-2e-4, 2e-4),
        rem + rng.uniform(-0.3, 0.3), step * (1.0 + rng.uniform(-2e-5, 2e-5)))


def _rates(mode, rng):
    prate, crate = rng.uniform(-1e-7, 1e-7), rng.uniform(0.0, 1e-9)
    return (prate if mode == "hd_full" else 0.0), (crate if mode in HD else 0.0)


def matrix_records(oracle, mode):
    """[channel][epoch] of the matrix launch; the same for every tap count and format."""
    def make():
        truth = _float_stream(oracle, "matrix")[1]
        rng = np.random.Generator(np.random.PCG64(8801))
        recs = ([], [])
        for start, (ch, n, res, tag) in zip(STARTS, WINDOWS):
            rem_carr, pstep, rem_code, cstep = _near_truth(truth[ch], start, rng)
            if tag == "fast":
                cstep = 0.5 + rng.uniform(0.0, 0.01)
            prate, crate = _rates(mode, rng)
            recs[ch].append(_rec(start - BIND[ch], n_of(n, tag, mode), tag, rem_carr, pstep, rem_code, cstep, prate, crate))
        return recs
    return _once(("recs", mode in HD, mode), make)


def _codes(oracle, mode, prns=PRNS):
    """Per channel: real chips; complex chips (the satellite's code and another one in quadrature); or test_16sc_gpu.py's int16 chips:
    (1, 0) on channel 0, (2, 1) on channel 1."""
    if mode == "complex":
        return [((ca_code(oracle, p) + 1j * ca_code(oracle, p + 3)) * np.float32(np.sqrt(0.5))).astype(np.complex64) for p in prns]
    if mode == "sc16":
        return [np.stack([ca_code(oracle, p) * (1 + ch), ca_code(oracle, p) * ch], 1).astype(np.int16) for ch, p in enumerate(prns)]
    return [ca_code(oracle, p) for p in prns]


def _long_code(mode, L):
    rng = np.random.Generator(np.random.PCG64(8184 + L))
    c = [(rng.integers(0, 2, L) * 2 - 1).astype(np.float32) for _ in range(2)]
    return ((c[0] + 1j * c[1]) * np.float32(np.sqrt(0.5))).astype(np.complex64) if mode == "complex" else c[0]


def matrix_launch(oracle, mode, fmt, n_taps):
    return Launch("matrix", mode, fmt, n_taps, 1023, 1023, _codes(oracle, mode), shifts_of(n_taps), "matrix", BIND, N_IQ, matrix_records(oracle, mode), SLICINGS, False)


RESYNC = [(m, f) for m, f in BATCH if m != "hd_full"]


def resync_launch(oracle, mode, fmt):
    """One record of 66 chunks + 77 samples at an odd start, one slice, 3 taps."""
    def recs():
        truth = _float_stream(oracle, "clean")[1]
        rem_carr, _, rem_code, cstep = _near_truth(truth[0], 1, np.random.Generator(np.random.PCG64(8802)))
        return ([_rec(1, RESYNC_N, "resync", rem_carr, 1.3, rem_code, cstep)],)
    return Launch("resync", mode, fmt, 3, 1023, 1023, _codes(oracle, mode)[:1], shifts_of(3), "clean", (0,), (N_CLEAN,), _once("resync", recs), (1,), False)


LDS_TABLE_FLOATS = 16000  # TRK_LDS_TABLE_FLOATS: a batch accepts codes of up to 16000 / words per chip - 64 chips
TABLE_L, TABLE_N = {"plain": 8184, "complex": 7936}, 4608  # (complex chips: the longest code a batch accepts)
TABLE_PATHS = [(m, f, t) for m in ("plain", "complex") for f in FORMATS for t in (3, 5)]


def table_launch(oracle, mode, fmt, n_taps):
    """Three records of one channel, L = 8184 (complex chips: 7936), N = 4608, 2 slices, records on the device (the host sizes the launch's LDS by the
    nominal window: below the table).  Nominal step: windowed.  Twice the nominal step: its slices fit neither.  3.3 x nominal and a
    code phase 7000 chips the other way: the window spans several periods, from a negative chip number."""
    L = TABLE_L[mode]

    def recs():
        rng = np.random.Generator(np.random.PCG64(8803))
        step = L / TABLE_N
        return ([_rec(off, TABLE_N, tag, rng.uniform(0, 6), rng.uniform(-0.01, 0.01), rem, k * step * (1.0 + rng.uniform(-1e-4, 1e-4)))
            for off, tag, rem, k in ((0, "nominal", 17.25, 1.0), (4611, "double", -4000.5, 2.0), (9005, "periods", 7000.75, 3.3))],)
    return Launch("table", mode, fmt, n_taps, L, L, [_long_code(mode, L)], shifts_of(n_taps), "clean", (0,), (N_CLEAN,), _once(("table", L), recs), (2,), True)


TINY_L = 31
TINY = [("plain", "f32"), ("complex", "f32")]


def tiny_launch(oracle, mode, fmt):
    """L = 31: a 140-sample window at half a chip per sample that starts on chip 30 -- cbase + span > 3 L, the `% L` fill loop -- and a
    nominal one."""
    def recs():
        return ([_rec(3, 140, "wrap", 1.0, 0.004, -30.2 + 0.7, 0.5), _rec(301, 200, "nominal", 2.0, -0.003, 4.4, 0.2557)],)
    return Launch("tiny", mode, fmt, 3, TINY_L, TINY_L, [_long_code(mode, TINY_L)], shifts_of(3), "clean", (0,), (N_CLEAN,), _once("tiny", recs), (1,), False)


LEVEL1_N = (513, 2597)
LEVEL1_MODES = MODES  # every overload: plain (flag off), 6-argument and 7-argument with the flag, Cpu_Multicorrelator, ..._16sc


def level1_call(oracle, mode, n_taps, n):
    """One level-1 call as a one-record launch: the input is the clean stream from sample 1 on (an odd sample of an aligned array)."""
    def recs():
        truth = _float_stream(oracle, "clean")[1]
        rng = np.random.Generator(np.random.PCG64(8804 + n + MODES.index(mode)))
        rem_carr, pstep, rem_code, cstep = _near_truth(truth[1], 1, rng)
        prate, crate = _rates(mode, rng)
        return ([_rec(1, n, "level1", rem_carr, pstep, rem_code, cstep, prate, crate)],)
    return Launch("level1", mode, "i16" if mode == "sc16" else "f32", n_taps, 1023, 1023, _codes(oracle, mode)[-1:], shifts_of(n_taps), "clean", (0,), (N_CLEAN,),
        _once(("level1", mode, n), recs), (1,), False)


def all_float_launches(oracle):
    """Every launch whose reference is the restatement."""
    for mode, fmt in BATCH:
        if mode != "sc16":
            for t in TAPS:
                yield matrix_launch(oracle, mode, fmt, t)
    for mode, fmt in RESYNC:
        if mode != "sc16":
            yield resync_launch(oracle, mode, fmt)
    for mode, fmt, t in TABLE_PATHS:
        yield table_launch(oracle, mode, fmt, t)
    for mode, fmt in TINY:
        yield tiny_launch(oracle, mode, fmt)
    for mode in LEVEL1_MODES:
        if mode != "sc16":
            for t in TAPS:
                for n in LEVEL1_N:
                    yield level1_call(oracle, mode, t, n)


# ---- references ----
def stream_fmt(launch):
    return "sc16" if launch.mode == "sc16" else launch.fmt


def scale_of(launch):
    return SCALE[stream_fmt(launch)]


def _key(launch):
    return (launch.table, launch.mode, launch.fmt, launch.n_taps, launch.recs[0][0].n)


def reference(oracle, launch):
    """[channel][epoch][tap] complex128: the float64 restatement on the format's samples; computed once, never modified."""
    def make():
        from open_loop_ref import correlate
        clean = samples(oracle, launch.stream, launch.fmt, launch.mode in HD)[1]
        return np.array([[correlate(oracle, clean[b + r.offset:], code, launch.shifts, r.params, launch.mode) for r in recs]
            for b, code, recs in zip(launch.binds, launch.codes, launch.recs)])
    return _once(("ref",) + _key(launch), make)


def compiled(oracle, launch):
    """The compiled oracle on the same input: [channel][epoch][tap] complex64, or for the 16-bit mode (int16 results [..., 2], exact
    int32 sums [..., 2])."""
    def make():
        q, clean = samples(oracle, launch.stream, stream_fmt(launch), launch.mode in HD)
        out = []
        for b, code, recs in zip(launch.binds, launch.codes, launch.recs):
            row = []
            for r in recs:
                a = [np.float32(r.args[k]) for k in ("rem_carr", "pstep", "rem_code", "cstep")]
                if launch.mode == "sc16":
                    row.append(oracle.multicorrelator_16sc(q[b + r.offset:], code, launch.shifts, a[0], a[1], a[2], a[3], r.n))
                elif launch.mode == "complex":
                    row.append(oracle.multicorrelator_cc(clean[b + r.offset:], code, launch.shifts, a[0], a[1], a[2], a[3], r.n))
                else:
                    row.append(oracle.multicorrelator(clean[b + r.offset:], code, launch.shifts, a[0], a[1], a[2], a[3], r.n,
                        phase_rate_step=np.float32(r.args["prate"]), code_rate_step=np.float32(r.args["crate"]), high_dyn=launch.mode in HD))
            out.append(row)
        if launch.mode == "sc16":
            return np.array([[r[0] for r in row] for row in out]), np.array([[r[1] for r in row] for row in out])
        return np.array(out)
    return _once(("orc",) + _key(launch), make)


def bars(oracle, launch):
    """[channel][epoch]: 1e-4 max_t |ref[t]| + NOISE scale sqrt(n); 0 for an empty window."""
    ref = reference(oracle, launch)
    return np.array([[REL * float(np.max(np.abs(ref[ch][k]))) + NOISE[launch.mode] * scale_of(launch) * np.sqrt(r.n) if r.n else 0.0
        for k, r in enumerate(recs)] for ch, recs in enumerate(launch.recs)])


# ---- the path of trk_epoch / trk_loop a record takes (trk_device.hpp restated: same formulas, float32 where the kernel's are) ----
def _chip_index(step, n, shift, rem):
    return int(np.floor((np.float32(step) * np.float32(n) + np.float32(shift)) - np.float32(rem)))


def _chip_index_hd(step, rate, n, shift0, rem):
    a = np.float32(step) * np.float32(n)
    r = np.float32(rate) * np.float32(np.uint32(n) * np.uint32(n))
    return int(np.floor(((a + r) + np.float32(shift0)) - np.float32(rem)))


def tap_delays(shifts, step):
    """The high-dynamics resampler's tap delays in samples (rintf of the shift differences over the step, accumulated)."""
    d, acc = [0], 0
    for t in range(1, len(shifts)):
        acc += int(np.rint((np.float32(shifts[t]) - np.float32(shifts[t - 1])) / np.float32(step)))
        d.append(acc)
    return d


def epoch_path(launch, ch, k, n_slices, lds_floats, align=ALIGN):
    """What trk_epoch decides for record k of channel ch: a, n_chunks, full[c], lc0, lc1 and per slice (c0, c1, table) with table one
    of "window" (filled with two conditional subtractions), "window_mod" (the `% L` fill loop), "lds_table" (whole table in LDS, modulo
    lookups), "global_table" (neither fits: lookups in global memory) -- and "none" for a slice without chunks."""
    r, L = launch.recs[ch][k], launch.code_len
    words = 2 if launch.mode == "complex" else 1
    hdr = launch.mode in HD
    p, shifts = r.params, launch.shifts
    a = (launch.binds[ch] + r.offset) % align
    N, V = r.n, r.n + a
    n_chunks = (V + CHUNK - 1) // CHUNK
    cps = (n_chunks + n_slices - 1) // n_slices
    room = max(launch.n_iq[ch] - r.offset, 0)
    path = dict(a=a, n_chunks=n_chunks, full=[(c > 0 or a == 0) and (c + 1) * CHUNK <= V for c in range(n_chunks)],
        lc0=0 if r.offset >= a else 1, lc1=min(n_chunks, (room + a) // CHUNK), slices=[])
    step, rem, rate = p.code_phase_step_chips, p.rem_code_phase_chips, p.code_phase_rate_step_chips
    for s in range(n_slices):
        c0 = s * cps
        c1 = min(n_chunks, c0 + cps)
        if hdr:
            n_lo, n_hi = 0, max(N - 1, 0)
            lo, hi = _chip_index_hd(step, rate, n_lo, shifts[0], rem), _chip_index_hd(step, rate, n_hi, shifts[0], rem)
            monotone = step > 0 and rate >= 0
        else:
            n_lo = max(c0 * CHUNK - a, 0)
            n_hi = max(min(c1 * CHUNK - a, N) - 1, n_lo)
            lo, hi = _chip_index(step, n_lo, min(shifts), rem), _chip_index(step, n_hi, max(shifts), rem)
            monotone = step >= 0
        span = hi - lo + 1
        if c0 >= c1:
            table = "none"
        elif monotone and span > 0 and span * words <= lds_floats:
            table = "window" if lo % L + span <= 3 * L else "window_mod"
        else:
            table = "lds_table" if L * words <= lds_floats else "global_table"
        path["slices"].append((c0, c1, table))
    return path
