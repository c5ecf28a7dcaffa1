"""GPU test of what depends on the arithmetic KIND of the tracking host code (gc_tracking.hip): the batched engine's four formats --
plain float chips, the high-dynamics variant, complex float chips, 16-bit complex chips with 16-bit input and output -- and the
level-1 correlator's three code kinds with their Carrier_wipeoff overloads.  Every entry point that accepts some kinds and refuses
others is called against a small object of each kind (2 channels, 3 taps, a 1023-chip code) with the expected status written
out, and the life cycles are walked: a format switch asks for every code again, a change of input format unbinds the inputs, a
round trip through another format gives the same bytes, a correlator that was freed or re-initialised gives the same bytes as a
fresh one.  Windows of 1000 samples (one workgroup) and 4500 samples (4 level-1 slices; with set_slices(2) the batch's partial-sum
path).  The literals pin the library's answers, so that a change of how the host stores the kind is seen to change none of them;
the results of the valid calls meet the CPU oracle as tests/test_tracking_gpu.py, test_complex_code_gpu.py and test_16sc_gpu.py
demand (1e-4 of |Prompt|; 16-bit: 3 LSB).

Of the six wrong pairings of code kind and arithmetic only five can be asked for through the C ABI: the 5-argument overload takes
its arithmetic (complex float or 16-bit) from the code that was set, so those two never meet each other; the 7- and 6-argument
overloads are tried with the high-dynamics flag set and cleared instead."""
import numpy as np
import pytest

from helpers import open_loop_params, rel_err, synth_stream
from test_16sc_gpu import MAX_LSB, _quantise
from test_tracking_gpu import TOL

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, 1, 4
FORMATS = ("plain", "high_dyn", "complex", "sc16")
L, FS, N_TAPS = 1023, 4_000_000, 3
WINDOWS = (1000, 4500)
SHIFTS = np.array([-0.5, 0.0, 0.5], np.float32)
CARR_RATE = np.float32(2 * np.pi * 50.0 / FS / FS)  # high-dynamics records: 50 Hz/s and a code rate term
CODE_RATE = np.float32(1e-12)

# entry point -> status per format, in the order of FORMATS; the message opens with the C function's name
TABLE = (
    ("set_code", "gc_trk_batch_set_code", (OK, OK, STATE, STATE)),
    ("set_code_complex", "gc_trk_batch_set_code_complex", (STATE, STATE, OK, STATE)),
    ("set_code_16sc", "gc_trk_batch_set_code_16sc", (STATE, STATE, STATE, OK)),
    ("set_complex_codes", "gc_trk_batch_set_complex_codes", (OK, STATE, OK, STATE)),
    ("set_16sc", "gc_trk_batch_set_16sc", (OK, STATE, STATE, OK)),
    ("set_input_format_f32", "gc_trk_batch_set_input_format", (OK, OK, OK, STATE)),
    ("set_input_format_i8", "gc_trk_batch_set_input_format", (OK, OK, OK, STATE)),
    ("set_input_format_i16", "gc_trk_batch_set_input_format", (OK, OK, OK, OK)),
    ("set_input_format_unknown", "gc_trk_batch_set_input_format", (INVALID, INVALID, INVALID, INVALID)),
    ("set_input_stream_other_format", "gc_trk_batch_set_input_stream", (INVALID, INVALID, INVALID, INVALID)),
    ("set_input_stream", "gc_trk_batch_set_input_stream", (OK, OK, OK, OK)),
    ("set_input_dev_misaligned", "gc_trk_batch_set_input_dev", (INVALID, INVALID, INVALID, INVALID)),
    ("set_input_dev", "gc_trk_batch_set_input_dev", (OK, OK, OK, OK)),
    ("run_without_code", "gc_trk_batch_run", (INVALID, INVALID, INVALID, INVALID)),
    ("run_without_input", "gc_trk_batch_run", (INVALID, INVALID, INVALID, INVALID)),
)


class Data:
    """Signal, codes, records and the oracle's sums, computed once and left unchanged."""

    def __init__(self, oracle):
        import gnsscorr
        import torch
        self.chips = [oracle.gps_l1_ca_code(prn).astype(np.float32) for prn in (3, 9)]
        self.sig, truth = synth_stream(self.chips, FS, 2 * max(WINDOWS) + 8, seed=411, cn0_db_hz=(62.0, 64.0))
        self.q = _quantise(self.sig, 4.0)
        self.d_sig = torch.from_numpy(self.sig.view(np.float32).copy()).cuda()
        self.d_q = torch.from_numpy(self.q).cuda()
        self.code = {
            "plain": self.chips,
            "high_dyn": self.chips,
            "complex": [(c * (1 + 0.25j)).astype(np.complex64) for c in self.chips],
            "sc16": [np.stack([c * (1 + ch), c * ch], 1).astype(np.int16) for ch, c in enumerate(self.chips)],
        }
        # channel ch correlates the window that starts at ch * n
        self.p = {n: [open_loop_params(truth[ch], FS, L, n, 2)[ch] for ch in range(2)] for n in WINDOWS}
        self.amp = [t["amp"] for t in truth]
        self.ref = {}
        for n in WINDOWS:
            for ch, p in enumerate(self.p[n]):
                a = (p["rem_carr"], p["phase_step"], p["rem_code"], p["code_step"], n)
                x, xq = self.sig[p["sample_offset"]:], self.q[p["sample_offset"]:]
                self.ref["plain", n, ch] = oracle.multicorrelator(x, self.chips[ch], SHIFTS, *a)
                self.ref["high_dyn", n, ch] = oracle.multicorrelator(x, self.chips[ch], SHIFTS, *a, phase_rate_step=CARR_RATE, code_rate_step=CODE_RATE,
                    high_dyn=True)
                self.ref["complex", n, ch] = oracle.multicorrelator_cc(x, self.code["complex"][ch], SHIFTS, *a)
                self.ref["sc16", n, ch] = oracle.multicorrelator_16sc(xq, self.code["sc16"][ch], SHIFTS, *a)
                # the 6-argument overload with the high-dynamics flag: plain rotator, resampler with the code rate term
                idx = oracle.resampler_indices(p["rem_code"], p["code_step"], SHIFTS, L, n, rate=CODE_RATE)
                wiped = x[:n].astype(np.complex128) * np.exp(-1j * (float(p["rem_carr"]) + float(p["phase_step"]) * np.arange(n)))
                self.ref["resampler", n, ch] = np.array([np.sum(wiped * self.chips[ch][idx[t]]) for t in range(N_TAPS)])
                assert abs(self.ref["plain", n, ch][1]) > 0.5 * self.amp[ch] * n  # the prompt correlator sees the signal
        self.gnsscorr = gnsscorr

    def records(self, fmt, n):
        g = self.gnsscorr
        rate = dict(carr_phase_rate_step_rad=float(CARR_RATE), code_phase_rate_step_chips=float(CODE_RATE)) if fmt == "high_dyn" else {}
        return g.epoch_params_array([[g.epoch_params(p["sample_offset"], float(p["rem_carr"]), float(p["phase_step"]), float(p["rem_code"]),
            float(p["code_step"]), n, **rate)] for p in self.p[n]])

    def check(self, fmt, n, ch, got):
        ref = self.ref[fmt, n, ch]
        if fmt == "sc16":
            ref, exact = ref
            want = ref.astype(np.int32) if np.array_equal(ref.astype(np.int32), exact) else np.clip(exact, -32768, 32767)
            assert np.abs(got.astype(np.int32) - want).max() <= MAX_LSB, (fmt, n, ch, got, want)
        elif fmt == "resampler":
            assert np.max(np.abs(got - ref)) <= TOL * abs(ref[1]), (fmt, n, ch, got, ref)
        else:
            assert rel_err(got, ref, 1) <= TOL, (fmt, n, ch, got, ref)


@pytest.fixture(scope="module")
def data(oracle):
    return Data(oracle)


def batch(gctx, fmt, max_code_length=L):
    import gnsscorr
    b = gnsscorr.TrackingBatch(gctx, 2, N_TAPS, max_code_length, high_dyn=(fmt == "high_dyn"))
    if fmt == "complex":
        b.set_complex_codes(True)
    if fmt == "sc16":
        b.set_16sc(True)
    return b


def set_codes(b, data, fmt):
    for ch in range(2):
        {"plain": b.set_code, "high_dyn": b.set_code, "complex": b.set_code_complex, "sc16": b.set_code_16sc}[fmt](ch, data.code[fmt][ch], SHIFTS)


def set_inputs(b, data, fmt):
    for ch in range(2):
        if fmt == "sc16":
            b.set_input_dev(ch, data.d_q.data_ptr(), data.q.shape[0])
        else:
            b.set_input_dev(ch, data.d_sig.data_ptr(), data.sig.size)


def status(fn, *args):
    """(status, message without the status prefix) of a call through the Python binding"""
    import gnsscorr
    try:
        fn(*args)
        return OK, ""
    except gnsscorr.GnsscorrError as e:
        return e.status, str(e).split(": ", 1)[1]


def call(gctx, b, data, fmt, entry):
    import gnsscorr
    own, other = (gnsscorr.GC_IQ_I16, gnsscorr.GC_IQ_F32) if fmt == "sc16" else (gnsscorr.GC_IQ_F32, gnsscorr.GC_IQ_I16)
    dev = data.d_q if fmt == "sc16" else data.d_sig
    if entry == "set_code":
        return status(b.set_code, 0, data.code["plain"][0], SHIFTS)
    if entry == "set_code_complex":
        return status(b.set_code_complex, 0, data.code["complex"][0], SHIFTS)
    if entry == "set_code_16sc":
        return status(b.set_code_16sc, 0, data.code["sc16"][0], SHIFTS)
    if entry == "set_complex_codes":
        return status(b.set_complex_codes, True)
    if entry == "set_16sc":
        return status(b.set_16sc, True)
    if entry.startswith("set_input_format_"):
        return status(b.set_input_format, {"f32": gnsscorr.GC_IQ_F32, "i16": gnsscorr.GC_IQ_I16, "i8": gnsscorr.GC_IQ_I8, "unknown": 99}[entry[17:]])
    if entry in ("set_input_stream", "set_input_stream_other_format"):
        ring = gnsscorr.IqStream(gctx, 16384, 4500, iq_format=own if entry == "set_input_stream" else other)
        try:
            return status(b.set_input_stream, 0, ring)
        finally:
            b.close()  # the batch's reference to the ring goes first
            ring.close()
    if entry == "set_input_dev_misaligned":
        return status(b.set_input_dev, 0, dev.data_ptr() + (2 if fmt == "sc16" else 4), 100)  # half a sample
    if entry == "set_input_dev":
        return status(b.set_input_dev, 0, dev.data_ptr(), 100)
    if entry == "run_without_code":
        set_inputs(b, data, fmt)
        return status(b.run, 1, data.records(fmt, 1000))
    if entry == "run_without_input":
        set_codes(b, data, fmt)
        return status(b.run, 1, data.records(fmt, 1000))
    raise AssertionError(entry)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_batch_entry_point_against_the_format(gctx, data, fmt):
    k = FORMATS.index(fmt)
    got = []
    for entry, c_name, want in TABLE:
        b = batch(gctx, fmt)
        try:
            st, text = call(gctx, b, data, fmt, entry)
            got.append((entry, st))
            assert st == OK or text.startswith(c_name + ":"), (entry, text)
        finally:
            b.close()
    assert got == [(entry, want[k]) for entry, _, want in TABLE]


def test_complex_chips_need_a_table_that_fits_twice(gctx):
    """2 * (max_code_length + 64) floats must fit the 16000-float LDS table; the high-dynamics refusal comes first"""
    import gnsscorr
    b = gnsscorr.TrackingBatch(gctx, 2, N_TAPS, 7936)  # 2 * 8000 = 16000: fits
    assert status(b.set_complex_codes, True)[0] == OK
    b.close()
    b = gnsscorr.TrackingBatch(gctx, 2, N_TAPS, 7937)
    st, text = status(b.set_complex_codes, True)
    assert st == INVALID and text.startswith("gc_trk_batch_set_complex_codes:")
    assert status(b.set_complex_codes, False)[0] == OK  # already real: nothing to do
    assert status(b.set_16sc, True)[0] == OK  # 4 bytes per chip: the table is as it was
    b.close()
    b = gnsscorr.TrackingBatch(gctx, 2, N_TAPS, 7937, high_dyn=True)
    assert status(b.set_complex_codes, True)[0] == STATE
    b.close()
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.TrackingBatch(gctx, 2, N_TAPS, 15937)  # 15937 + 64 > 16000
    assert e.value.status == INVALID


def run_all(b, data, fmt):
    """the batch's result bytes: both windows, the longer one also whole and in two slices (the partial-sum path), each against the oracle"""
    out = []
    for n, slices in ((1000, 0), (4500, 0), (4500, 1), (4500, 2)):
        b.set_slices(slices)
        got = b.run(1, data.records(fmt, n))
        assert got.shape == ((2, 1, N_TAPS, 2) if fmt == "sc16" else (2, 1, N_TAPS))
        for ch in range(2):
            data.check(fmt, n, ch, got[ch, 0])
        out.append(got.tobytes())
    b.set_slices(0)
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_results_meet_the_oracle_and_repeat(gctx, data, fmt):
    b = batch(gctx, fmt)
    set_codes(b, data, fmt)
    set_inputs(b, data, fmt)
    first = run_all(b, data, fmt)
    assert run_all(b, data, fmt) == first
    b.close()


def needs(b, data, fmt, what):
    """gc_trk_batch_run checks the records against the channels' inputs first, then every channel's code"""
    st, text = status(b.run, 1, data.records(fmt, 1000))
    want = {"code": "gc_trk_batch_run: channel 0 has no code", "input": "gc_trk_batch_run: job 0 window [0, +1000) exceeds the channel's 0 samples"}[what]
    assert st == INVALID and text.startswith(want), text


@pytest.mark.parametrize("other", ["complex", "sc16"])
def test_a_format_switch_asks_for_the_codes_again_and_a_round_trip_gives_the_same_bytes(gctx, data, other):
    switch = {"complex": lambda b, on: b.set_complex_codes(on), "sc16": lambda b, on: b.set_16sc(on)}[other]
    b = batch(gctx, "plain")
    set_codes(b, data, "plain")
    set_inputs(b, data, "plain")
    first = run_all(b, data, "plain")
    switch(b, False)  # the format it already has: nothing is dropped
    assert run_all(b, data, "plain") == first
    switch(b, True)
    if other == "sc16":
        needs(b, data, other, "input")  # the 16-bit switch goes through the input format: float samples are unbound
        set_inputs(b, data, other)
    needs(b, data, other, "code")
    set_codes(b, data, other)
    there = run_all(b, data, other)  # complex chips: the float inputs stayed bound
    fresh = batch(gctx, other)
    set_codes(fresh, data, other)
    set_inputs(fresh, data, other)
    assert run_all(fresh, data, other) == there
    fresh.close()
    switch(b, True)  # again: nothing is dropped
    assert run_all(b, data, other) == there
    switch(b, False)
    if other == "sc16":
        needs(b, data, "plain", "input")
        set_inputs(b, data, "plain")
    needs(b, data, "plain", "code")
    set_codes(b, data, "plain")
    assert run_all(b, data, "plain") == first
    b.close()


def test_a_change_of_input_format_unbinds_the_inputs(gctx, data):
    import gnsscorr
    b = batch(gctx, "plain")
    set_codes(b, data, "plain")
    set_inputs(b, data, "plain")
    first = run_all(b, data, "plain")
    b.set_input_format(gnsscorr.GC_IQ_F32)  # no change: the inputs stay
    assert run_all(b, data, "plain") == first
    b.set_input_format(gnsscorr.GC_IQ_I16)
    needs(b, data, "plain", "input")
    b.set_input_format(gnsscorr.GC_IQ_F32)
    needs(b, data, "plain", "input")
    set_inputs(b, data, "plain")  # the codes stayed
    assert run_all(b, data, "plain") == first
    b.close()


# ---- level 1 ----
KINDS = ("real", "real_high_dyn", "complex", "sc16")


def correlator(gctx, kind):
    import gnsscorr
    c = {"complex": gnsscorr.HipMulticorrelator, "sc16": gnsscorr.HipMulticorrelator16sc}.get(kind, gnsscorr.HipMulticorrelatorRealCodes)(gctx)
    if kind.startswith("real"):
        c.set_high_dynamics_resampler(kind == "real_high_dyn")
    return c


def set_code(c, data, kind, ch=0):
    c.set_local_code_and_taps(L, data.code[{"real": "plain", "real_high_dyn": "plain"}.get(kind, kind)][ch], SHIFTS.copy())


def set_vectors(c, data, kind, n, ch=0):
    off = data.p[n][ch]["sample_offset"]
    out = np.zeros((N_TAPS, 2), np.int16) if kind == "sc16" else np.zeros(N_TAPS, np.complex64)
    c.set_input_output_vectors(out, data.q[off:] if kind == "sc16" else data.sig[off:])
    return out


def wipeoff(c, data, kind, n, overload=None, ch=0):
    """status of the kind's own overload (or of `overload`: 7, 6 or 5 arguments) through the C ABI"""
    import gnsscorr
    lib, p = gnsscorr.load_library(), data.p.get(n, data.p[1000])[ch]
    a = (float(p["rem_carr"]), float(p["phase_step"]), float(p["rem_code"]), float(p["code_step"]))
    overload = overload or (7 if kind.startswith("real") else 5)
    if overload == 7:
        rate = (float(CARR_RATE), float(CODE_RATE)) if kind == "real_high_dyn" else (0.0, 0.0)
        return lib.gc_correlator_carrier_wipeoff_multicorrelator_resampler(c._h, a[0], a[1], rate[0], a[2], a[3], rate[1], n)
    if overload == 6:
        return lib.gc_correlator_carrier_wipeoff_multicorrelator_resampler_6(c._h, a[0], a[1], a[2], a[3], float(CODE_RATE) if kind == "real_high_dyn" else 0.0, n)
    return lib.gc_correlator_carrier_wipeoff_multicorrelator_resampler_5(c._h, a[0], a[1], a[2], a[3], n)


def test_a_wipeoff_needs_init_code_and_vectors_in_any_order(gctx, data):
    for kind in KINDS:
        c = correlator(gctx, kind)
        assert wipeoff(c, data, kind, 1000) == STATE  # before init
        c.init(4500, N_TAPS)
        assert wipeoff(c, data, kind, 1000) == STATE  # before the code setter
        set_code(c, data, kind)
        assert wipeoff(c, data, kind, 1000) == STATE  # before the vector setter
        set_vectors(c, data, kind, 1000)
        assert wipeoff(c, data, kind, 1000) == OK
        assert wipeoff(c, data, kind, 4500) == OK
        assert wipeoff(c, data, kind, 4501) == INVALID  # more than init() sized the object for
        assert wipeoff(c, data, kind, -1) == INVALID
        c.free()
        assert wipeoff(c, data, kind, 1000) == STATE
        c.close()


def test_code_kind_against_overload_and_vectors(gctx, data):
    import gnsscorr
    float_vectors = gnsscorr.HipMulticorrelatorRealCodes.set_input_output_vectors
    short_vectors = gnsscorr.HipMulticorrelator16sc.set_input_output_vectors
    lib = gnsscorr.load_library()
    fout, sout = np.zeros(N_TAPS, np.complex64), np.zeros((N_TAPS, 2), np.int16)
    got = []
    for kind in ("real", "complex", "sc16"):
        for overload in (7, 6, 5):
            for high_dyn in (0, 1):
                for vectors in ("float", "short"):
                    c = correlator(gctx, kind)
                    assert lib.gc_correlator_set_high_dynamics_resampler(c._h, high_dyn) == OK
                    c.init(4500, N_TAPS)
                    set_code(c, data, kind)
                    if vectors == "float":
                        float_vectors(c, fout, data.sig)
                    else:
                        short_vectors(c, sout, data.q)
                    got.append((kind, overload, high_dyn, vectors, wipeoff(c, data, kind, 1000, overload)))
                    c.close()
    want = []
    for kind in ("real", "complex", "sc16"):
        for overload in (7, 6, 5):
            for high_dyn in (0, 1):
                for vectors in ("float", "short"):
                    # the 7- and 6-argument overloads correlate real chips, the 5-argument one whichever complex chips were set;
                    # 16-bit chips go with 16-bit vectors, float chips with float vectors
                    fits = (kind == "real") == (overload != 5) and (kind == "sc16") == (vectors == "short")
                    want.append((kind, overload, high_dyn, vectors, OK if fits else STATE))
    assert got == want


def test_a_code_longer_than_the_lds_table_of_its_kind(gctx, data):
    """L + 64 floats (complex chips: twice that) must fit 16000"""
    shifts = np.zeros(N_TAPS, np.float32)
    for kind, longest in (("real", 15936), ("complex", 7936), ("sc16", 15936)):
        c = correlator(gctx, kind)
        c.init(4500, N_TAPS)
        set_vectors(c, data, kind, 1000)
        code = {"real": np.ones(longest + 1, np.float32), "complex": np.ones(longest + 1, np.complex64), "sc16": np.ones((longest + 1, 2), np.int16)}[kind]
        c.set_local_code_and_taps(longest + 1, code, shifts)
        assert wipeoff(c, data, kind, 1000) == INVALID
        c.set_local_code_and_taps(0, code, shifts)
        assert wipeoff(c, data, kind, 1000) == INVALID
        c.close()


def level1_bytes(c, data, kind, check=True):
    """result bytes of the kind's calls: both windows, both channels' codes; real chips: the 7- and the 6-argument overload"""
    out = []
    for n in WINDOWS:
        for ch in range(2):
            set_code(c, data, kind, ch)
            res = set_vectors(c, data, kind, n, ch)
            for overload in ((7, 6) if kind.startswith("real") else (5,)):
                assert wipeoff(c, data, kind, n, overload, ch) == OK
                if check:
                    fmt = {"real": "plain", "real_high_dyn": "resampler" if overload == 6 else "high_dyn"}.get(kind, kind)
                    data.check(fmt, n, ch, res)
                out.append(res.tobytes())
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_level1_results_meet_the_oracle_whatever_the_objects_history(gctx, data, kind):
    c = correlator(gctx, kind)
    c.init(4500, N_TAPS)
    fresh = level1_bytes(c, data, kind)
    assert level1_bytes(c, data, kind, check=False) == fresh
    c.close()
    c = correlator(gctx, kind)
    c.init(1000, N_TAPS)
    set_code(c, data, kind)
    set_vectors(c, data, kind, 1000)
    assert wipeoff(c, data, kind, 1000) == OK
    assert wipeoff(c, data, kind, 4500) == INVALID
    c.init(6000, N_TAPS)  # init() on an initialised object: released and sized again; the pointers that were set stay
    assert wipeoff(c, data, kind, 4500) == OK
    assert level1_bytes(c, data, kind, check=False) == fresh
    c.free()
    assert wipeoff(c, data, kind, 1000) == STATE
    c.init(4500, N_TAPS)
    assert wipeoff(c, data, kind, 4500) == OK
    assert level1_bytes(c, data, kind, check=False) == fresh
    c.free()
    c.free()  # nothing left to release
    c.close()
