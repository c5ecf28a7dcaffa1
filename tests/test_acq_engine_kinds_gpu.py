"""GPU test of what depends on the KIND of an acquisition engine (plain, paired, QuickSync, Tong, CAF; gc_acquisition.hip): every
entry point that accepts some kinds and refuses others, against one small engine of each kind -- 500 samples per ms, 1 ms, one
satellite slot, five Doppler bins (QuickSync: 500 samples per code folded twice) -- with the expected status written out, and the
life cycle every kind shares: a dwell without a code is a call-sequence error, a reset engine reads as zeros, and a search
repeated after a reset gives the same bytes.  The literals pin the library's answers, so that a change of how the host tells the
kinds apart (AcqKind and ACQ_KIND_TRAITS, csrc/acq_engine_sizes.h) is seen to change none of them; a refusal is GC_ERR_INVALID
whichever check gives it, and its text starts with the name of the function called."""
import numpy as np
import pytest

from test_acquisition_gpu import _conf

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, 1, 4
SPM, DMAX, DSTEP = 500, 1000, 500
KINDS = ("plain", "paired", "quicksync", "tong", "caf")
FIELDS = ("indext", "doppler_hz", "doppler_index", "test_statistics", "mag", "input_power", "second_peak", "second_peak_full_row", "acq_delay_samples",
    "acq_doppler_hz")

# (entry point, C function whose name opens the message) -> status per kind, in the order of KINDS
TABLE = (
    ("set_local_code", "gc_acq_set_local_code", (OK, INVALID, OK, OK, INVALID)),
    ("set_local_code_pair", "gc_acq_set_local_code_pair", (INVALID, OK, INVALID, INVALID, INVALID)),
    ("set_local_code_iq", "gc_acq_set_local_code_iq", (INVALID, INVALID, INVALID, INVALID, OK)),
    ("set_local_code_iq_without_q", "gc_acq_set_local_code_iq", (INVALID, INVALID, INVALID, INVALID, INVALID)),  # the CAF engine searches both components
    ("set_step_two_on", "gc_acq_set_step_two", (OK, OK, INVALID, INVALID, INVALID)),
    ("set_step_two_off", "gc_acq_set_step_two", (OK, OK, INVALID, INVALID, INVALID)),
    ("set_frequency_offset", "gc_acq_set_frequency_offset", (OK, OK, INVALID, INVALID, INVALID)),
    ("set_threshold", "gc_acq_tong_set_threshold", (INVALID, INVALID, INVALID, OK, INVALID)),
    ("tong_status", "gc_acq_tong_status", (INVALID, INVALID, INVALID, OK, INVALID)),
    ("tong_search_stream", "gc_acq_tong_search_stream", (INVALID, INVALID, INVALID, OK, INVALID)),
    ("caf_vectors", "gc_acq_caf_vectors", (INVALID, INVALID, INVALID, INVALID, OK)),
    ("candidates", "gc_acq_quicksync_candidates", (INVALID, INVALID, OK, INVALID, INVALID)),
)


def engine(gctx, kind):
    import gnsscorr
    fs = SPM * 1000
    if kind == "plain":
        acq = gnsscorr.PcpsAcquisition(gctx, 1, make_2_steps=True, num_doppler_bins_step2=4, **_conf(fs, 1, 1, float(SPM), DMAX, DSTEP))
        want = (SPM, SPM, 4)  # ceil(2 * 1000 / 500): the plain grid leaves +doppler_max out
    elif kind == "paired":
        acq = gnsscorr.PcpsAcquisition(gctx, 1, combine="max", make_2_steps=True, num_doppler_bins_step2=4, **_conf(fs, 1, 1, float(SPM), DMAX, DSTEP))
        want = (SPM, SPM, 4)
    elif kind == "quicksync":
        acq = gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=2, **_conf(fs, 2, 1, float(SPM), DMAX, DSTEP))
        want = (SPM // 2, 2 * SPM, 5)
    elif kind == "tong":
        acq = gnsscorr.PcpsAcquisition(gctx, 1, tong=(2, 4, 3), **_conf(fs, 1, 1, float(SPM), DMAX, DSTEP))
        want = (SPM, SPM, 5)
    else:
        acq = gnsscorr.PcpsAcquisition(gctx, 1, caf=dict(both_components=1, hypotheses=2, window_hz=1000, arithmetic="exact"),
            **_conf(fs, 1, 1, float(SPM), DMAX, DSTEP))
        want = (SPM, SPM, 5)
    assert (acq.fft_size, acq.consumed_samples, acq.num_doppler_bins) == want
    return acq


def codes():
    rng = np.random.Generator(np.random.PCG64(11))
    return [(rng.integers(0, 2, 2 * SPM) * 2.0 - 1.0).astype(np.complex64) for _ in range(2)]


def block():
    rng = np.random.Generator(np.random.PCG64(12))
    return (rng.standard_normal(2 * SPM) + 1j * rng.standard_normal(2 * SPM)).astype(np.complex64)


def set_codes(acq, kind):
    a, b = codes()
    if kind == "paired":
        acq.set_local_code_pair(0, a, b)
    elif kind == "caf":
        acq.set_local_code_iq(0, a, b)
    else:
        acq.set_local_code(0, a)


def call(gctx, acq, kind, entry):
    import gnsscorr
    a, b = codes()
    if entry == "set_local_code":
        acq.set_local_code(0, a)
    elif entry == "set_local_code_pair":
        acq.set_local_code_pair(0, a, b)
    elif entry == "set_local_code_iq":
        acq.set_local_code_iq(0, a, b)
    elif entry == "set_local_code_iq_without_q":
        acq.set_local_code_iq(0, a)
    elif entry == "set_step_two_on":
        acq.set_step_two(True, 250.0)
        assert acq.num_doppler_bins == 4
    elif entry == "set_step_two_off":
        acq.set_step_two(False)
    elif entry == "set_frequency_offset":
        acq.set_frequency_offset(1250)
    elif entry == "set_threshold":
        acq.set_threshold(2.5)
    elif entry == "tong_status":
        st = acq.tong_status()
        assert [(s.state, s.tong_count, s.dwell_count) for s in st] == [(0, 2, 0)]
    elif entry == "tong_search_stream":
        ring = gnsscorr.IqStream(gctx, 4096, 2 * SPM)
        try:
            ring.push(block())
            if kind == "tong":
                set_codes(acq, kind)
            res, st = acq.tong_search_stream(ring, 0, 1)
            assert len(res) == 1 and st[0].dwell_count == 1
        finally:
            ring.close()
    elif entry == "caf_vectors":
        assert not any(np.any(v) for v in acq.caf_vectors(0))
    elif entry == "candidates":
        delay, val = acq.candidates(0)
        assert delay.size == 2 and not np.any(delay) and not np.any(val)
    else:
        raise AssertionError(entry)


@pytest.mark.parametrize("kind", KINDS)
def test_every_entry_point_against_the_kind(gctx, kind):
    import gnsscorr
    k = KINDS.index(kind)
    got = []
    for entry, c_name, want in TABLE:
        acq = engine(gctx, kind)
        try:
            call(gctx, acq, kind, entry)
            got.append((entry, OK))
        except gnsscorr.GnsscorrError as e:
            got.append((entry, e.status))
            text = str(e).split(": ", 1)[1]
            assert text.startswith(c_name + ":"), (entry, text)
        finally:
            acq.close()
    assert got == [(entry, want[k]) for entry, _, want in TABLE]


@pytest.mark.parametrize("kind", KINDS)
def test_a_dwell_before_any_code_is_a_sequence_error(gctx, kind):
    import gnsscorr
    acq = engine(gctx, kind)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        acq.dwell(block())
    assert e.value.status == STATE
    acq.close()


def _snapshot(acq, res):
    return tuple(getattr(res[0], f) for f in FIELDS), acq.grid(0).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_reset_reads_as_zeros_and_a_repeated_search_gives_the_same_bytes(gctx, kind):
    acq = engine(gctx, kind)
    set_codes(acq, kind)
    x = block()
    first = _snapshot(acq, acq.dwell(x))
    assert np.any(np.frombuffer(first[1], np.float32))
    acq.reset()
    res = acq.fetch_results()
    if kind in ("tong", "caf"):
        assert tuple(getattr(res[0], f) for f in FIELDS) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert not np.any(acq.grid(0))
    again = _snapshot(acq, acq.dwell(x))
    assert again == first
    acq.close()
