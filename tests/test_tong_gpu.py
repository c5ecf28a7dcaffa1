"""GPU tests of the Tong engine (gc_acq_create_tong; pcps_tong_acquisition_cc.cc) against the numpy restatement tests/tong_ref.py.
Bars are those of tests/test_acquisition_gpu.py: indices and Doppler exact, magnitudes within TOL = 1e-4 of the peak.  Seeds and
thresholds are chosen on the restatement alone (tests/tong_cases.py) under two conditions every test asserts before it touches the
GPU: every q_d = d_mag / dwell_count lies at least 1e-2 (50 x the 2 TOL the engine's mag may be off) from the threshold, which sits
in the geometric middle of a gap of ratio >= 1.05 between sorted q values; and a result's cell is compared exactly only where the
restatement's top cell beats its runner-up by more than 10 TOL -- otherwise any cell it holds within TOL of its maximum is accepted.
The sizes here (N = 2000, 4000, 6625, 25000 and the five-satellite engine's 2000) reach the column sizes N1 = 2, 4, 5 and 25 only; the
column kernel at every instantiated N1 is tests/test_acq_kind_matrix_gpu.py's."""
import numpy as np
import pytest

import tong_cases as tc
import tong_ref
from tong_cases import TOL

pytestmark = pytest.mark.gpu

FIELDS = ("indext", "doppler_index", "doppler_hz", "mag", "test_statistics", "input_power", "acq_delay_samples", "acq_doppler_hz", "second_peak",
    "second_peak_full_row")
TONG = (2, 4, 8)
PRN = 7
# N -> (seed, which of the allowed thresholds).  On the restatement: 2000 misses twice (negative at dwell 2, frozen through dwell 3),
# 4000 walks up, down, up, 6625 hits twice (positive at dwell 2, frozen through dwell 3), 25000 walks down, up, up
SHAPES = {2000: (1, 0), 4000: (1, 0), 6625: (3, 0), 25000: (1, 0)}
# five satellites in one engine: 46 / 44 / 43 / 42 dB-Hz and an absent PRN; 26 bins (6250 / 500, inclusive), so that a satellite's
# inter-pass cells are 416 KB and GNSSCORR_ACQ_Q_MB = 1 makes batches of 2 + 2 + 1
FIVE_PRNS, FIVE_CN0, FIVE_SEED, FIVE_N, FIVE_DMAX = (3, 7, 12, 19, 25), (46.0, 44.0, 43.0, 42.0), 239, 2000, 6250
FIVE_BLOCKS = 12


def _fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


def _status(s):
    return (s.state, s.tong_count, s.dwell_count)


_REF = {}


def matrix_reference(oracle, N):
    if N not in _REF:
        seed, which = SHAPES[N]
        x = tc.signal(oracle, N, (PRN,), (44.0,), 3, seed)
        code = tc.codes(oracle, N, (PRN,))[0]
        recs = tong_ref.search(oracle, x, [code], N * 1000, N, tc.DMAX, tc.DSTEP, 3)
        thr, ratio = tc.thresholds(recs)[which]
        for r in recs[0]:
            r.grid.setflags(write=False)
        _REF[N] = (x, code, recs[0], thr, ratio)
    return _REF[N]


def five_reference(oracle):
    if "five" not in _REF:
        N = FIVE_N
        x = tc.signal(oracle, N, FIVE_PRNS[:4], FIVE_CN0, FIVE_BLOCKS, FIVE_SEED)
        codes = tc.codes(oracle, N, FIVE_PRNS)
        recs = tong_ref.search(oracle, x, codes, N * 1000, N, FIVE_DMAX, 500, TONG[2])
        # the lowest allowed threshold under which the five satellites end in all three ways at three different dwells
        chosen = None
        for thr, ratio in tc.thresholds(recs):
            outs = [tc.outcome(r, thr, TONG)[-1] for r in recs]
            positive = any(s[0] == tong_ref.POSITIVE for s in outs)
            by_count = any(s[0] == tong_ref.NEGATIVE and s[1] == 0 and s[2] < TONG[2] for s in outs)
            by_dwells = any(s[0] == tong_ref.NEGATIVE and s[1] != 0 and s[2] == TONG[2] for s in outs)
            if positive and by_count and by_dwells and len({s[2] for s in outs}) >= 3:
                chosen = (thr, ratio, outs)
                break
        assert chosen is not None
        for rs in recs:
            for r in rs:
                r.grid.setflags(write=False)
        _REF["five"] = (x, codes, recs) + chosen
    return _REF["five"]


def five_engine(gctx, codes, threshold, n_sats=5):
    import gnsscorr
    acq = gnsscorr.PcpsAcquisition(gctx, n_sats, tong=TONG, **tc.conf(FIVE_N, FIVE_DMAX, 500))
    assert (acq.fft_size, acq.consumed_samples, acq.num_doppler_bins) == (FIVE_N, FIVE_N, 26)
    for s_, c in enumerate(codes[:n_sats]):
        acq.set_local_code(s_, c)
    acq.set_threshold(threshold)
    return acq


def five_ring(gctx, x, iq_format=None):
    import gnsscorr
    kw = {} if iq_format is None else dict(iq_format=iq_format)
    ring = gnsscorr.IqStream(gctx, capacity_samples=(FIVE_BLOCKS + 2) * FIVE_N, max_window_samples=FIVE_N, **kw)
    ring.push(x)
    return ring


def snapshot(acq, res, status):
    """Everything a caller can read of every satellite, for bit-exact comparisons."""
    return [(_fields(res[s_]), _status(status[s_]), acq.grid(s_).tobytes(), acq.peek(acq.PEEK_ROW_MAX, s_).tobytes()) for s_ in range(acq.n_sats)]


# ---- 1. four walks against the restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", list(SHAPES))
def test_matrix_against_the_restatement(gctx, oracle, N):
    """Four sizes (column sizes N1 = 2, 4, 5 and 25), one per kind of walk: no matrix of the column kernel's instances, in spite of
    the name.  All 17 N1 of acq_cols_tong_kernel run in tests/test_acq_kind_matrix_gpu.py."""
    import gnsscorr
    x, code, recs, thr, ratio = matrix_reference(oracle, N)
    walk = tc.outcome(recs, thr, TONG)
    margin = tc.decision_margin([recs], thr)
    print("restatement: threshold %.6g in a gap of ratio %.3f, decision margin %.3g, walk %s" % (thr, ratio, margin, walk))
    assert ratio >= 1.05 and margin >= 1e-2
    bins = tong_ref.doppler_bins(tc.DMAX, tc.DSTEP)
    acq = gnsscorr.PcpsAcquisition(gctx, 1, tong=TONG, **tc.conf(N))
    assert (acq.fft_size, acq.consumed_samples, acq.num_doppler_bins) == (N, N, 5)
    acq.set_local_code(0, code)
    assert _status(acq.tong_status()[0]) == (tong_ref.RUNNING, TONG[0], 0) and not np.any(acq.grid(0))
    acq.set_threshold(thr)
    for d in range(3):
        res = acq.dwell(x[d * N:(d + 1) * N])
        # a satellite that has decided keeps everything of its deciding dwell
        at = min(d, len(walk) - 1)
        tc.check_dwell(acq, 0, recs[at], acq.tong_status()[0], res[0], walk[at], bins, N)
    acq.close()


# ---- 2. independent termination ----------------------------------------------------------------------------------------------------

def test_satellites_terminate_independently(gctx, oracle):
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    margin = tc.decision_margin(recs, thr)
    print("restatement: threshold %.6g in a gap of ratio %.3f, decision margin %.3g, outcomes %s" % (thr, ratio, margin, outs))
    assert ratio >= 1.05 and margin >= 1e-2
    bins = tong_ref.doppler_bins(FIVE_DMAX, 500)
    ring = five_ring(gctx, x)
    acq = five_engine(gctx, codes, thr)
    res, status = acq.tong_search_stream(ring, 0)
    assert [_status(s) for s in status] == outs and [_status(s) for s in acq.tong_status()] == outs
    for s_ in range(5):
        tc.check_dwell(acq, s_, recs[s_][outs[s_][2] - 1], status[s_], res[s_], outs[s_], bins, FIVE_N)
    full = snapshot(acq, res, status)
    _REF["five_snapshot"] = full
    # a second engine stopped at a satellite's deciding dwell holds, bit for bit, what the first one still holds of it: nothing
    # written by the later dwells shows
    for D in sorted({o[2] for o in outs}):
        other = five_engine(gctx, codes, thr)
        r2, s2 = other.tong_search_stream(ring, 0, D)
        stopped = snapshot(other, r2, s2)
        for s_ in range(5):
            if outs[s_][2] == D:
                assert stopped[s_] == full[s_], (s_, D)
            elif outs[s_][2] > D:
                assert stopped[s_][1] == (tong_ref.RUNNING, tc.outcome(recs[s_], thr, TONG)[D - 1][1], D) and stopped[s_][2] != full[s_][2], (s_, D)
        other.close()
    acq.close()
    ring.close()


# ---- 3. satellite batches ------------------------------------------------------------------------------------------------------------

def test_satellite_batches_are_bit_identical(gctx, oracle, monkeypatch):
    """GNSSCORR_ACQ_Q_MB = 1 (read when the engine is created): batches of 2 + 2 + 1 satellites, each with its own slice of the
    frozen flags, against the single batch of the default."""
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    assert ratio >= 1.05 and tc.decision_margin(recs, thr) >= 1e-2
    ring = five_ring(gctx, x)
    out = []
    for q_mb in (None, "1"):
        if q_mb is None:
            monkeypatch.delenv("GNSSCORR_ACQ_Q_MB", raising=False)
        else:
            monkeypatch.setenv("GNSSCORR_ACQ_Q_MB", q_mb)
        acq = five_engine(gctx, codes, thr)
        res, status = acq.tong_search_stream(ring, 0)
        out.append(snapshot(acq, res, status))
        acq.close()
    ring.close()
    assert [s[1] for s in out[0]] == outs
    for s_ in range(5):
        assert out[1][s_] == out[0][s_], s_


# ---- 4. ways of driving the search ----------------------------------------------------------------------------------------------------

def test_ways_of_driving_the_search(gctx, oracle):
    import torch
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    assert ratio >= 1.05 and tc.decision_margin(recs, thr) >= 1e-2
    N = FIVE_N
    ring = five_ring(gctx, x)
    a = five_engine(gctx, codes, thr)
    one_call = snapshot(a, *a.tong_search_stream(ring, 0))
    assert [s[1] for s in one_call] == outs
    # more dwells are not run once tong_max_dwells is reached: a further call changes nothing
    assert snapshot(a, *a.tong_search_stream(ring, TONG[2] * N, 3)) == one_call
    a.close()
    b = five_engine(gctx, codes, thr)
    for d in range(TONG[2]):
        res, status = b.tong_search_stream(ring, d * N, 1)
        assert max(s.dwell_count for s in status) == d + 1
    assert snapshot(b, res, status) == one_call
    b.close()
    c = five_engine(gctx, codes, thr)
    d_x = torch.from_numpy(np.array(x[:TONG[2] * N]).view(np.float32)).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for d in range(TONG[2]):
        c.dwell_enqueue(d_x.data_ptr() + 8 * N * d, st.cuda_stream)
        c.flush(st.cuda_stream)
    res = c.fetch_results(st.cuda_stream)
    assert snapshot(c, res, c.tong_status()) == one_call
    c.close()
    ring.close()
    # a ring that does not hold all the blocks asked for is refused before anything runs
    import gnsscorr
    short = gnsscorr.IqStream(gctx, capacity_samples=8 * N, max_window_samples=N)
    short.push(x[:3 * N])
    e = five_engine(gctx, codes, thr)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        e.tong_search_stream(short, 0)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    assert [_status(s) for s in e.tong_status()] == [(tong_ref.RUNNING, TONG[0], 0)] * 5
    res, status = e.tong_search_stream(short, 0, 3)
    assert max(s.dwell_count for s in status) == 3
    e.close()
    short.close()


# ---- 5. reset ------------------------------------------------------------------------------------------------------------------------

def test_reset_between_two_searches(gctx, oracle):
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    N = FIVE_N
    ring = five_ring(gctx, x)
    a = five_engine(gctx, codes, thr)
    first = snapshot(a, *a.tong_search_stream(ring, 0))
    a.reset()
    assert [_status(s) for s in a.tong_status()] == [(tong_ref.RUNNING, TONG[0], 0)] * 5
    assert not np.any(a.grid(0)) and not np.any(a.grid(4))
    second = snapshot(a, *a.tong_search_stream(ring, 4 * N))
    fresh = five_engine(gctx, codes, thr)
    want = snapshot(fresh, *fresh.tong_search_stream(ring, 4 * N))
    assert second == want and second != first
    fresh.close()
    a.close()
    ring.close()


# ---- 6. input formats ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt, scale", [("GC_IQ_I16", 200.0), ("GC_IQ_I8", 20.0)])
def test_integer_rings(gctx, oracle, fmt, scale):
    import gnsscorr
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    dt, lo, hi = (np.int16, -32768, 32767) if fmt == "GC_IQ_I16" else (np.int8, -128, 127)
    q = np.clip(np.round(np.array(x).view(np.float32) * scale), lo, hi).astype(dt)
    xf = q.astype(np.float32).view(np.complex64)
    ring_f = five_ring(gctx, xf)
    a = five_engine(gctx, codes, thr, n_sats=3)
    want = snapshot(a, *a.tong_search_stream(ring_f, 0))
    a.close()
    ring_f.close()
    ring_q = five_ring(gctx, q.reshape(-1, 2), iq_format=getattr(gnsscorr, fmt))
    b = five_engine(gctx, codes, thr, n_sats=3)
    b.set_input_format(getattr(gnsscorr, fmt))
    assert snapshot(b, *b.tong_search_stream(ring_q, 0)) == want
    b.close()
    ring_q.close()


# ---- 7. an all-zero first block ----------------------------------------------------------------------------------------------------------

def test_all_zero_first_block(gctx, oracle):
    """P = 0: s is infinite, every cell 0 * inf = NaN, no cell wins a comparison: d_mag and the statistic are 0, the counter goes
    down; NaN stays in the accumulated grid, so the next dwell counts down as well and the search ends negative."""
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    N = FIVE_N
    a = five_engine(gctx, codes, thr, n_sats=2)
    r = a.dwell(np.zeros(N, np.complex64))
    for s_ in range(2):
        assert (r[s_].mag, r[s_].test_statistics, r[s_].input_power) == (0.0, 0.0, 0.0)
        assert (r[s_].indext, r[s_].doppler_index, r[s_].doppler_hz, r[s_].acq_delay_samples) == (0, 0, 0, 0.0)
    assert [_status(s) for s in a.tong_status()] == [(tong_ref.RUNNING, 1, 1)] * 2
    r = a.dwell(x[:N])
    assert [_status(s) for s in a.tong_status()] == [(tong_ref.NEGATIVE, 0, 2)] * 2
    assert r[0].mag == 0.0 and r[0].test_statistics == 0.0 and r[0].input_power > 0.0
    a.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(gctx, oracle):
    import gnsscorr
    x, codes, recs, thr, ratio, outs = five_reference(oracle)
    for bad in ((0, 2, 3), (2, 2, 3), (3, 2, 3), (1, 2, 0)):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            gnsscorr.PcpsAcquisition(gctx, 1, tong=bad, **tc.conf(FIVE_N))
        assert ei.value.status == gnsscorr.GC_ERR_INVALID, bad
    for kw in (dict(bit_transition_flag=True), dict(make_2_steps=True)):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            gnsscorr.PcpsAcquisition(gctx, 1, tong=TONG, **tc.conf(FIVE_N, **kw))
        assert ei.value.status == gnsscorr.GC_ERR_INVALID, kw
    a = gnsscorr.PcpsAcquisition(gctx, 1, tong=TONG, **tc.conf(FIVE_N, dstep=0))
    assert a.num_doppler_bins == 9  # a step of 0 means 250
    a.set_local_code(0, codes[0])
    for call in (lambda: a.set_step_two(True, 0.0), lambda: a.set_frequency_offset(1000), lambda: a.set_local_code_pair(0, codes[0], codes[0])):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            call()
        assert ei.value.status == gnsscorr.GC_ERR_INVALID
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **tc.conf(FIVE_N))
    for call in (lambda: plain.set_threshold(1.0), plain.tong_status):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            call()
        assert ei.value.status == gnsscorr.GC_ERR_INVALID
    plain.close()
    # the default threshold is +inf: every dwell counts down
    a.dwell(x[:FIVE_N])
    a.dwell(x[FIVE_N:2 * FIVE_N])
    assert _status(a.tong_status()[0]) == (tong_ref.NEGATIVE, 0, 2)
    a.close()
