"""GPU tests of the CAF engine (gc_acq_create_caf; galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc) against the numpy restatement
tests/caf_ref.py.  Bars are those of tests/test_acquisition_gpu.py: indices and Doppler exact, magnitudes within TOL = 1e-4 of the
peak.  Seeds are chosen on the restatement alone (tests/caf_cases.py) under preconditions every test asserts before it touches the
GPU: EVERY choice of hypothesis has a relative margin >= 1e-2 (engine values may be 2 TOL off; under REFERENCE arithmetic the margin
holds for every index the QB maximum may be read at), a Doppler is compared only where the CAF argmax has a margin >= 1e-2, and a
cell is compared exactly only where the top cell beats its runner-up by more than 10 TOL (tests/tong_cases.py)."""
import numpy as np
import pytest

import caf_cases as cc
import caf_ref
from caf_cases import TOL

pytestmark = pytest.mark.gpu

FIELDS = ("indext", "doppler_index", "doppler_hz", "mag", "test_statistics", "input_power", "acq_delay_samples", "acq_doppler_hz", "second_peak",
    "second_peak_full_row")
SPM = 2000
BINS = caf_ref.doppler_bins(cc.DMAX, cc.DSTEP)


def _fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


def snapshot(acq, res):
    """Everything a caller can read of every satellite, for bit-exact comparisons."""
    return [(_fields(res[s]), acq.grid(s).tobytes(), acq.peek(acq.PEEK_ROW_MAX, s).tobytes()) + tuple(v.tobytes() for v in acq.caf_vectors(s))
        for s in range(acq.n_sats)]


def engine(gctx, spm, ms, n_sats=1, dmax=cc.DMAX, dstep=cc.DSTEP, conf_kw=None, **caf):
    import gnsscorr
    acq = gnsscorr.PcpsAcquisition(gctx, n_sats, caf=caf, **cc.conf(spm, ms, dmax, dstep, **(conf_kw or {})))
    assert (acq.fft_size, acq.consumed_samples, acq.num_doppler_bins) == (spm * ms, spm * ms, len(caf_ref.doppler_bins(dmax, dstep)))
    return acq


# ---- 1. the matrix against the restatement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cc.MATRIX, ids=[c.name for c in cc.MATRIX])
def test_matrix_against_the_restatement(gctx, oracle, case):
    x, ci, cq, rec = cc.matrix_reference(oracle, case)
    ok, text = cc.preconditions(rec, case)
    print("restatement, seed %d: %s, top-cell margin %.3g (recorded: %s)" % (case.seed, text, cc.top_cell_margin(rec), case.recorded))
    assert ok
    acq = engine(gctx, case.spm, case.ms, **cc.caf_kw(case))
    assert not any(np.any(v) for v in acq.caf_vectors(0)) and not np.any(acq.grid(0))
    acq.set_local_code_iq(0, ci, cq if case.both else None)
    # the replicas as the engine holds them: conj(FFT) of IA, QA, IB, QB
    reps = caf_ref.replicas(ci, cq if case.both else None, case.both, case.hyp, case.spm)
    assert len(reps) == case.R
    for i, rep in enumerate(reps):
        want = np.conj(oracle.fft(rep))
        assert np.max(np.abs(acq.peek(acq.PEEK_CODE, i) - want)) <= TOL * np.max(np.abs(want)), i
    res = acq.dwell(x)
    caf = cc.check_dwell(acq, 0, rec, res[0], BINS, case.spm)
    # the filter on the engine's own CAF_I / CAF_Q is test 2; against the restatement's it holds to the vectors' error, away from
    # REFERENCE's cancelling sums
    if case.arithmetic == caf_ref.EXACT:
        assert np.max(np.abs(caf - rec.caf)) <= 4 * TOL * float(np.max(rec.grid))
    acq.close()


# ---- 2. the filter, bit for bit ------------------------------------------------------------------------------------------------------

_NINE = {}


def nine_bins(oracle):
    if not _NINE:
        x = cc.signal(cc.PRN, SPM, 2 * SPM, 31, signs_i=(-1, 1), doppler=-330.0)
        _NINE["x"] = x
        _NINE["codes"] = cc.local_codes(cc.PRN, SPM, 2)
    return _NINE["x"], _NINE["codes"]


@pytest.mark.parametrize("arithmetic", ["reference", "exact"])
@pytest.mark.parametrize("H", [1, 2])
def test_filter_is_bit_exact_on_the_device(gctx, oracle, arithmetic, H):
    """CAF_I and CAF_Q read back, caf_ref's filter on THOSE vectors: CAF equal bit for bit; nine bins (1000 / 250)."""
    x, (ci, cq) = nine_bins(oracle)
    mode = caf_ref.REFERENCE if arithmetic == "reference" else caf_ref.EXACT
    for both in (1, 0):
        acq = engine(gctx, SPM, 2, dmax=1000, dstep=250, both_components=both, hypotheses=2, window_hz=500 * H, arithmetic=arithmetic)
        assert acq.num_doppler_bins == 9
        acq.set_local_code_iq(0, ci, cq if both else None)
        res = acq.dwell(x)
        caf, caf_i, caf_q, _ = acq.caf_vectors(0)
        assert np.all(caf_i > 0) and (np.all(caf_q > 0) if both else not np.any(caf_q))
        want = caf_ref.caf_filter(caf_i, caf_q if both else None, H, mode)
        assert np.array_equal(caf.view(np.uint32), want.view(np.uint32)), (caf, want)
        d = caf_ref.first_max(want)
        bins = caf_ref.doppler_bins(1000, 250)
        assert (res[0].doppler_index, res[0].doppler_hz, res[0].acq_doppler_hz) == (d, bins[d], float(bins[d]))
        acq.close()


# ---- 3. the bit-transition keep rule --------------------------------------------------------------------------------------------------

def test_bit_transition_keep_rule(gctx, oracle):
    N = 2 * SPM
    parts = [cc.signal(cc.PRN, SPM, N, 20 + d, amp=(a, a), doppler=f, delay=300 + 111 * d, signs_i=(1, 1)) for d, (a, f) in enumerate(((0.4, 450.0), (0.25, -60.0), (0.15, -930.0)))]
    x = np.concatenate(parts)
    ci, cq = cc.local_codes(cc.PRN, SPM, 2)
    (recs,) = caf_ref.search(oracle, x, [(ci, cq)], 1000 * SPM, N, cc.DMAX, cc.DSTEP, 1, 2, cc.WINDOW, caf_ref.EXACT, samples_per_code=SPM, bit_transition=True, n_dwells=3)
    case = cc.Case("keep", SPM, 2, 1, 2, caf_ref.EXACT, 0)
    for r in recs:
        ok, text = cc.preconditions(r, case)
        print(text)
        assert ok
    assert recs[0].mag > 1.5 * recs[1].mag > 2.0 * recs[2].mag and [r.doppler_hz for r in recs] == [500, 0, -1000]
    acq = engine(gctx, SPM, 2, conf_kw=dict(bit_transition_flag=True, max_dwells=3), both_components=1, hypotheses=2, window_hz=cc.WINDOW, arithmetic="exact")
    acq.set_local_code_iq(0, ci, cq)
    first = None
    for _ in range(2):
        out = []
        for d in range(3):
            res = acq.dwell(x[d * N:(d + 1) * N])
            cc.check_dwell(acq, 0, recs[d], res[0], BINS, SPM, cell_of_this_dwell=(d == 0))
            out.append(_fields(res[0]))
        # the cell fields and the statistic stay those of the first dwell; mag, input_power and the Doppler follow each dwell
        assert out[1][0] == out[0][0] == out[2][0] and out[1][4] == out[0][4] == out[2][4] and out[0][6] == out[1][6] == out[2][6] == 300.0
        assert out[0][3] > out[1][3] > out[2][3] and len({o[5] for o in out}) == 3 and [o[2] for o in out] == [500, 0, -1000]
        if first is None:
            first = out
            acq.reset()  # starts over: the same three dwells give the same three results, bit for bit
            assert _fields(acq.fetch_results()[0]) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) and not np.any(acq.grid(0))
    assert out == first
    # without the flag every dwell's own cell is reported
    free = engine(gctx, SPM, 2, both_components=1, hypotheses=2, window_hz=0, arithmetic="exact")
    free.set_local_code_iq(0, ci, cq)
    assert [free.dwell(x[d * N:(d + 1) * N])[0].acq_delay_samples for d in range(3)] == [300.0, 411.0, 522.0]
    free.close()
    acq.close()


# ---- 4. satellite batches ----------------------------------------------------------------------------------------------------------------

FIVE_PRNS = (3, 11, 19, 24, 30)
_FIVE = {}


def five(oracle):
    """Five satellites, four present, three bins (500 / 500) at N = 4000 and R = 4: a satellite's inter-pass cells are 384 KB, so
    GNSSCORR_ACQ_Q_MB = 1 makes batches of 2 + 2 + 1."""
    if not _FIVE:
        N = 2 * SPM
        x = np.zeros(N, np.complex128)
        for i, prn in enumerate(FIVE_PRNS[:4]):
            x = x + cc.signal(prn, SPM, N, 50 + i, amp=(0.2 + 0.03 * i, 0.2), doppler=-400.0 + 250.0 * i, signs_i=((-1, 1), (1, 1))[i % 2], noise=(i == 0))
        x = x.astype(np.complex64)
        x.setflags(write=False)
        _FIVE["x"] = x
        _FIVE["codes"] = [cc.local_codes(p, SPM, 2) for p in FIVE_PRNS]
    return _FIVE["x"], _FIVE["codes"]


def five_engine(gctx, codes, n_sats=5, arithmetic="reference"):
    acq = engine(gctx, SPM, 2, n_sats=n_sats, dmax=500, dstep=500, both_components=1, hypotheses=2, window_hz=1000, arithmetic=arithmetic)
    for s, (ci, cq) in enumerate(codes[:n_sats]):
        acq.set_local_code_iq(s, ci, cq)
    return acq


def test_satellite_batches_are_bit_identical(gctx, oracle, monkeypatch):
    x, codes = five(oracle)
    out = []
    for q_mb in (None, "1"):
        if q_mb is None:
            monkeypatch.delenv("GNSSCORR_ACQ_Q_MB", raising=False)
        else:
            monkeypatch.setenv("GNSSCORR_ACQ_Q_MB", q_mb)
        acq = five_engine(gctx, codes)
        out.append(snapshot(acq, acq.dwell(x)))
        acq.close()
    for s in range(5):
        assert out[1][s] == out[0][s], s
    # the four satellites present are found at their delays' bins; the fifth is not the same as any of them
    assert len({o[1] for o in out[0]}) == 5


# ---- 5. ways of driving a dwell ------------------------------------------------------------------------------------------------------

def test_ways_of_driving_a_dwell(gctx, oracle):
    import gnsscorr
    import torch
    x, codes = five(oracle)
    N = 2 * SPM
    a = five_engine(gctx, codes, n_sats=3)
    want = snapshot(a, a.dwell(x))
    d_x = torch.from_numpy(np.array(x).view(np.float32)).cuda()
    torch.cuda.synchronize()
    assert snapshot(a, a.dwell_dev(d_x.data_ptr())) == want
    st = torch.cuda.Stream()
    a.dwell_enqueue(d_x.data_ptr(), st.cuda_stream)
    a.flush(st.cuda_stream)
    assert snapshot(a, a.fetch_results(st.cuda_stream)) == want
    ring = gnsscorr.IqStream(gctx, capacity_samples=4 * N, max_window_samples=N)
    ring.push(np.zeros(123, np.complex64))
    ring.push(x)
    assert snapshot(a, a.dwell_stream(ring, 123)) == want
    ring.close()
    a.close()


@pytest.mark.parametrize("fmt, scale", [("GC_IQ_I16", 200.0), ("GC_IQ_I8", 20.0)])
def test_integer_rings(gctx, oracle, fmt, scale):
    """A cshort / cbyte ring against the restatement on the dequantised samples."""
    import gnsscorr
    case = cc.MATRIX[1]
    x, ci, cq, _ = cc.matrix_reference(oracle, case)
    dt, lo, hi = (np.int16, -32768, 32767) if fmt == "GC_IQ_I16" else (np.int8, -128, 127)
    q = np.clip(np.round(np.array(x).view(np.float32) * scale), lo, hi).astype(dt)
    xf = q.astype(np.float32).view(np.complex64)
    ((rec,),) = caf_ref.search(oracle, xf, [(ci, cq)], 1000 * case.spm, case.N, cc.DMAX, cc.DSTEP, case.both, case.hyp, cc.WINDOW, case.arithmetic,
        samples_per_code=case.spm)
    ok, text = cc.preconditions(rec, case)
    print(text)
    assert ok
    ring = gnsscorr.IqStream(gctx, capacity_samples=4 * case.N, max_window_samples=case.N, iq_format=getattr(gnsscorr, fmt))
    ring.push(q.reshape(-1, 2))
    acq = engine(gctx, case.spm, case.ms, **cc.caf_kw(case))
    acq.set_local_code_iq(0, ci, cq)
    acq.set_input_format(getattr(gnsscorr, fmt))
    res = acq.dwell_stream(ring, 0)
    cc.check_dwell(acq, 0, rec, res[0], BINS, case.spm)
    acq.close()
    ring.close()


# ---- 6. degenerate slots ------------------------------------------------------------------------------------------------------------------

def test_one_replica_is_the_plain_engine(gctx, oracle):
    """R = 1, no filter: grid, row maxima and result of a plain gc_acq_create engine (single dwell, no bit transition, the CFAR
    statistic max / N^4 / P), bit for bit where both compute the same thing."""
    import gnsscorr
    x = cc.signal(cc.PRN, SPM, SPM, 5, amp=(0.3, 0.0), doppler=-420.0)
    ci, _ = cc.local_codes(cc.PRN, SPM, 1)
    plain = gnsscorr.PcpsAcquisition(gctx, 1, num_doppler_bins_override=5, **cc.conf(SPM, 1))
    plain.set_local_code(0, ci)
    p = plain.dwell(x)[0]
    acq = engine(gctx, SPM, 1, both_components=0, hypotheses=1, window_hz=0, arithmetic="reference")
    acq.set_local_code_iq(0, ci)
    r = acq.dwell(x)[0]
    assert acq.grid(0).tobytes() == plain.grid(0).tobytes()
    assert acq.peek(acq.PEEK_ROW_MAX, 0).tobytes() == plain.peek(plain.PEEK_ROW_MAX, 0).tobytes()
    assert (r.indext, r.doppler_index, r.doppler_hz, r.acq_delay_samples) == (p.indext, p.doppler_index, p.doppler_hz, p.acq_delay_samples)
    assert r.input_power == p.input_power and abs(r.test_statistics - p.test_statistics) <= 1e-6 * p.test_statistics
    caf, caf_i, caf_q, choice = acq.caf_vectors(0)
    assert np.array_equal(caf_i, acq.peek(acq.PEEK_ROW_MAX, 0)[:, 0]) and not np.any(caf) and not np.any(caf_q) and not np.any(choice)
    plain.close()
    acq.close()


def test_equal_hypotheses_choose_a(gctx, oracle):
    """One code period per block: B is A negated as a whole, the planes are equal and `>=` keeps A in every bin (EXACT arithmetic:
    REFERENCE would hold QA against the I plane)."""
    x = cc.signal(cc.PRN, SPM, SPM, 5, doppler=-420.0)
    ci, cq = cc.local_codes(cc.PRN, SPM, 1)
    out = []
    for hyp in (2, 1):
        acq = engine(gctx, SPM, 1, both_components=1, hypotheses=hyp, window_hz=1000, arithmetic="exact")
        acq.set_local_code_iq(0, ci, cq)
        out.append(snapshot(acq, acq.dwell(x)))
        assert not np.any(acq.caf_vectors(0)[3])
        acq.close()
    assert out[0] == out[1]


# ---- 7. an all-zero block ----------------------------------------------------------------------------------------------------------------

def test_all_zero_block(gctx, oracle):
    """P = 0: every plane is zero, no cell wins against d_mag = 0, the kept statistic and the cell fields stay as they were and no NaN
    is written into kept state."""
    case = cc.MATRIX[1]
    x, ci, cq, rec = cc.matrix_reference(oracle, case)
    acq = engine(gctx, case.spm, case.ms, conf_kw=dict(bit_transition_flag=True, max_dwells=2), **cc.caf_kw(case, window=0))
    acq.set_local_code_iq(0, ci, cq)
    z = acq.dwell(np.zeros(case.N, np.complex64))[0]
    assert _fields(z) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert not np.any(acq.grid(0)) and not any(np.any(v) for v in acq.caf_vectors(0))
    r = acq.dwell(x)[0]
    assert r.mag > 0 and r.test_statistics > 0 and np.isfinite(r.test_statistics)
    z = acq.dwell(np.zeros(case.N, np.complex64))[0]
    assert (z.mag, z.input_power) == (0.0, 0.0)
    assert (z.test_statistics, z.indext, z.doppler_index, z.doppler_hz, z.acq_delay_samples) == (r.test_statistics, r.indext, r.doppler_index, r.doppler_hz,
        r.acq_delay_samples)
    acq.close()


# ---- 8. what is refused on a handle ------------------------------------------------------------------------------------------------------

def test_refusals_on_handles(gctx, oracle):
    import gnsscorr
    ci, cq = cc.local_codes(cc.PRN, SPM, 2)
    acq = engine(gctx, SPM, 2, both_components=1, hypotheses=2, window_hz=1000, arithmetic="reference")
    calls = (lambda: acq.set_local_code(0, ci), lambda: acq.set_local_code_pair(0, ci, cq), lambda: acq.set_step_two(True, 0.0),
        lambda: acq.set_frequency_offset(1000), lambda: acq.set_local_code_iq(0, ci), lambda: acq.set_local_code_iq(1, ci, cq))
    for i, call in enumerate(calls):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            call()
        assert ei.value.status == gnsscorr.GC_ERR_INVALID, i
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        acq.dwell(np.zeros(2 * SPM, np.complex64))  # no local code yet
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    acq.close()
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **cc.conf(SPM, 1))
    for call in (lambda: plain.set_local_code_iq(0, ci, cq), lambda: plain.caf_vectors(0)):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            call()
        assert ei.value.status == gnsscorr.GC_ERR_INVALID
    plain.close()
    # the refusals of gc_acq_create_caf, with a context this time
    bad = (dict(hypotheses=3), dict(hypotheses=0), dict(arithmetic="fast"), dict(both_components=2), dict(window_hz=999), dict(window_hz=5000))
    for kw in bad:
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            gnsscorr.PcpsAcquisition(gctx, 1, caf=kw, **cc.conf(SPM, 2))
        assert ei.value.status == gnsscorr.GC_ERR_INVALID, kw
    for ckw in (dict(make_2_steps=True), dict(bit_transition_flag=True, max_dwells=0), dict(dstep=0), dict(dmax=5000, dstep=1)):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            gnsscorr.PcpsAcquisition(gctx, 1, caf={}, **cc.conf(SPM, 2, **ckw))
        assert ei.value.status == gnsscorr.GC_ERR_INVALID, ckw
    # 2001 bins (10000 / 10) are inside the limit
    big = gnsscorr.PcpsAcquisition(gctx, 1, caf=dict(window_hz=100), **cc.conf(500, 1, 10000, 10))
    assert big.num_doppler_bins == 2001
    big.close()
