"""GPU tests of the QuickSync engine (gc_acq_create_quicksync; pcps_quicksync_acquisition_cc.cc) against the numpy restatement
tests/quicksync_ref.py.  Bars are those of tests/test_acquisition_gpu.py: indices and Doppler exact, magnitudes within TOL = 1e-4 of
the peak.  The restatement of a shape is computed once, shared and read-only."""
import ctypes as C

import numpy as np
import pytest

import quicksync_ref
from test_acquisition_gpu import TOL, _conf

pytestmark = pytest.mark.gpu

FIELDS = ("indext", "doppler_index", "doppler_hz", "mag", "test_statistics", "input_power", "acq_delay_samples", "acq_doppler_hz", "second_peak",
    "second_peak_full_row")
DMAX, DSTEP = 1000, 500  # five bins, both ends included
PRN = 7

# (N, f) -> seed of helpers.synth_stream.  Seeds are chosen on the restatement alone (its preconditions below hold, and for the
# divisible shapes it finds the true delay in the nearest bin): with f code periods integrated coherently a Doppler half way between
# two bins 500 Hz apart is lost altogether for f = 4, whatever the implementation.
SHAPES = {(2000, 2): 1, (4000, 2): 1, (4000, 4): 3, (4000, 3): 1, (5000, 4): 3, (16000, 2): 2, (25000, 4): 2}
SHAPE_IDS = ["N%d-f%d" % k for k in SHAPES]


def _fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


def _qs_conf(N, f, dmax=DMAX, dstep=DSTEP, **kw):
    fs = N * 1000
    return _conf(fs, f, 1, float(N), dmax, dstep, **kw)


def _signal(oracle, N, f, seed, n_blocks=1, prns=(PRN,)):
    from helpers import synth_stream
    return synth_stream([oracle.gps_l1_ca_code(p).astype(np.float32) for p in prns], N * 1000, n_blocks * f * N, seed=seed, cn0_db_hz=(47.0, 47.0), doppler_max=900.0)


_REF = {}


def reference(oracle, N, f):
    """Per shape, once: the signal, its truth, the sampled code and the restatement's result."""
    if (N, f) not in _REF:
        x, truth = _signal(oracle, N, f, SHAPES[(N, f)])
        code = oracle.gps_l1_ca_code_sampled(PRN, N * 1000)[:N]
        (r,) = quicksync_ref.search(oracle, x, [code], N * 1000, N, f, DMAX, DSTEP)
        r.grid.setflags(write=False)
        x.setflags(write=False)
        _REF[(N, f)] = (x, truth[0], code, r)
    return _REF[(N, f)]


def preconditions(r):
    """On the restatement alone: (top cell - second cell) / top cell, best candidate / runner-up."""
    flat = np.sort(r.grid.ravel())
    margin = float((flat[-1] - flat[-2]) / flat[-1])
    vals = sorted(r.corr_output_f)
    ratio = float(vals[-1] / vals[-2]) if len(vals) > 1 else float("inf")
    return margin, ratio


# ---- 1. the matrix against the restatement ----------------------------------------------------------------------------------------

def check_against_the_restatement(gctx, oracle, N, f, case, truth_checked):
    """One engine, one dwell of `case` = (x, truth, code, restatement's result) for a code period of N samples folded f times: the
    grid, row maxima, result, candidates and delay, the folded code spectrum and a wipe-off row.  Shared with
    tests/test_acq_kind_matrix_gpu.py; returns the engine for what a caller runs on top (the caller closes it)."""
    import gnsscorr
    x, truth, code, ref = case
    M, L = N // f, f * N
    margin, ratio = preconditions(ref)
    print("restatement: k* %d bin %d delay %d, margin %.3g, candidate ratio %.3g" % (ref.indext, ref.doppler_index, ref.acq_delay_samples, margin, ratio))
    assert margin > 10 * TOL and ratio >= 2.0
    if truth_checked:
        # the true delay and the nearest bin; (4000, 3) folds 1333-sample pieces of 4000-sample periods and slips a sample per period
        expect = (-truth["tau0"] * N * 1000 / 1.023e6) % N
        d = abs(ref.acq_delay_samples - expect)
        assert min(d, N - d) <= N / 1023.0 + 1
        assert abs(ref.doppler_hz - truth["doppler"]) <= DSTEP / 2
    acq = gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=f, **_qs_conf(N, f))
    assert (acq.fft_size, acq.consumed_samples, acq.num_doppler_bins) == (M, L, 5)
    acq.set_local_code(0, code)
    r = acq.dwell(x)[0]
    grid = acq.grid(0)
    peak = ref.grid.max()
    assert grid.shape == ref.grid.shape
    err = float(np.max(np.abs(grid - ref.grid)) / peak)
    print("grid error %.3g of the peak" % err)
    assert err <= TOL
    rows = acq.peek(acq.PEEK_ROW_MAX, 0)
    for b, (val, idx) in enumerate(ref.row_max):
        assert abs(rows[b, 0] - val) <= TOL * peak, b
        # the position is the reference's, or a cell the reference holds within TOL of its row maximum
        assert int(rows[b, 1]) == idx or abs(ref.grid[b, int(rows[b, 1])] - val) <= TOL * peak, b
    assert int(rows[ref.doppler_index, 1]) == ref.indext
    assert (r.indext, r.doppler_index, r.doppler_hz, r.acq_doppler_hz) == (ref.indext, ref.doppler_index, ref.doppler_hz, float(ref.doppler_hz))
    assert abs(r.mag - ref.mag) <= 2 * TOL * ref.mag
    assert abs(r.input_power - ref.input_power) <= 2 * TOL * ref.input_power
    assert abs(r.test_statistics - ref.test_statistics) <= 2 * TOL * ref.test_statistics
    assert r.second_peak == 0.0 and r.second_peak_full_row == 0.0
    delay, val = acq.candidates(0)
    print("candidates", delay.tolist(), val.tolist(), ref.corr_output_f)
    assert delay.tolist() == ref.possible_delay
    assert np.max(np.abs(val.astype(np.float64) - np.array(ref.corr_output_f))) <= TOL * max(ref.corr_output_f)
    assert r.acq_delay_samples == float(ref.acq_delay_samples)
    # the intermediates a failure would be traced through
    w = acq.peek(acq.PEEK_WIPEOFF, 3)
    # sincosf of the GPU and of the host libm may differ in the last bit; the running phase itself is exact
    assert w.size == L and np.max(np.abs(w - quicksync_ref.wipeoffs(oracle, N * 1000, [500], L)[0])) <= 2e-6
    cf = np.conj(oracle.fft(quicksync_ref.fold(code, M, f)))
    got = acq.peek(acq.PEEK_CODE, 0)
    assert got.size == M and np.max(np.abs(got - cf)) <= TOL * np.max(np.abs(cf))
    assert acq.peek(acq.PEEK_SPECTRUM, 2).size == M
    return acq


@pytest.mark.parametrize("N, f", list(SHAPES), ids=SHAPE_IDS)
def test_matrix_against_the_restatement(gctx, oracle, N, f):
    check_against_the_restatement(gctx, oracle, N, f, reference(oracle, N, f), N % f == 0).close()


# ---- 2. f = 1 is the plain search --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [2000, 4000])
def test_f1_against_the_plain_engine(gctx, oracle, N):
    """No folding: M = N, L = N.  With the bin count overridden to the plain engine's four (-1000 .. 500) both search the same cells:
    grids within TOL, indices and Doppler exact, and the single candidate is k* itself."""
    import gnsscorr
    x, truth = _signal(oracle, N, 1, seed=31 + N)
    code = oracle.gps_l1_ca_code_sampled(PRN, N * 1000)[:N]
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **_qs_conf(N, 1))
    qs = gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=1, **_qs_conf(N, 1, num_doppler_bins_override=4))
    assert (plain.fft_size, plain.num_doppler_bins) == (N, 4) and (qs.fft_size, qs.consumed_samples, qs.num_doppler_bins) == (N, N, 4)
    plain.set_local_code(0, code)
    qs.set_local_code(0, code)
    r0, r1 = plain.dwell(x)[0], qs.dwell(x)[0]
    g0, g1 = plain.grid(0), qs.grid(0)
    assert np.max(np.abs(g1 - g0)) <= TOL * g0.max()
    assert (r1.indext, r1.doppler_index, r1.doppler_hz) == (r0.indext, r0.doppler_index, r0.doppler_hz)
    assert abs(r1.mag - r0.mag) <= 2 * TOL * r0.mag and abs(r1.test_statistics - r0.test_statistics) <= 2 * TOL * r0.test_statistics
    assert abs(r1.input_power - r0.input_power) <= 2 * TOL * r0.input_power
    delay, val = qs.candidates(0)
    assert delay.tolist() == [r1.indext] and r1.acq_delay_samples == float(r1.indext) and val[0] > 0.0
    assert abs(r1.doppler_hz - truth[0]["doppler"]) <= DSTEP
    plain.close()
    qs.close()


# ---- 3. batches of satellites ----------------------------------------------------------------------------------------------------

def test_satellite_batches(gctx, oracle, monkeypatch):
    """N = 16000, f = 2, 21 bins (5000 / 500, inclusive): a satellite's inter-pass cells are 1.3 MB, so GNSSCORR_ACQ_Q_MB = 1 (read when
    the engine is created) runs the three slots one at a time and the default all at once: not a bit may differ.  Two slots hold
    PRNs of the signal, the third an absent one."""
    import gnsscorr
    N, f = 16000, 2
    prns = (5, 23, 14)
    x, truth = _signal(oracle, N, f, seed=5, prns=prns[:2])
    out = []
    for q_mb in (None, "1"):
        if q_mb is None:
            monkeypatch.delenv("GNSSCORR_ACQ_Q_MB", raising=False)
        else:
            monkeypatch.setenv("GNSSCORR_ACQ_Q_MB", q_mb)
        acq = gnsscorr.PcpsAcquisition(gctx, 3, folding_factor=f, **_qs_conf(N, f, 5000, 500))
        assert (acq.fft_size, acq.num_doppler_bins) == (8000, 21)
        for s_, p in enumerate(prns):
            acq.set_local_code(s_, oracle.gps_l1_ca_code_sampled(p, N * 1000)[:N])
        res = acq.dwell(x)
        out.append(([_fields(r) for r in res], [acq.grid(s_) for s_ in range(3)], [tuple(a.tolist() for a in acq.candidates(s_)) for s_ in range(3)]))
        acq.close()
    assert out[1][0] == out[0][0] and out[1][2] == out[0][2]
    for s_ in range(3):
        assert np.array_equal(out[1][1][s_], out[0][1][s_]), s_
    stats = [fl[FIELDS.index("test_statistics")] for fl in out[0][0]]
    print("statistics", stats, [(t["doppler"], t["tau0"]) for t in truth])
    assert stats[2] < min(stats[0], stats[1])
    # every slot has its own winner and its own candidates
    assert out[0][2][0] != out[0][2][1]


# ---- 4. input paths --------------------------------------------------------------------------------------------------------------

def test_input_paths(gctx, oracle):
    import gnsscorr
    import torch
    N, f = 4000, 2
    L = f * N
    x, _ = _signal(oracle, N, f, seed=SHAPES[(N, f)], n_blocks=3)
    code = oracle.gps_l1_ca_code_sampled(PRN, N * 1000)[:N]

    def engine():
        a = gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=f, **_qs_conf(N, f))
        a.set_local_code(0, code)
        return a

    def snapshot(a, res):
        return (_fields(res[0]), a.grid(0).tobytes(), tuple(v.tolist() for v in a.candidates(0)))

    acq = engine()
    want = snapshot(acq, acq.dwell(x))
    # two runs: the same bits
    assert snapshot(acq, acq.dwell(x)) == want
    # enqueue + fetch on a caller's stream
    d_x = torch.from_numpy(x.view(np.float32).copy()).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    acq.dwell_enqueue(d_x.data_ptr(), st.cuda_stream)
    assert snapshot(acq, acq.fetch_results(st.cuda_stream)) == want
    assert snapshot(acq, acq.dwell_dev(d_x.data_ptr())) == want
    # a second dwell on another block does not carry the first one's grid: it equals a fresh engine's
    second = snapshot(acq, acq.dwell(x[L:]))
    fresh = engine()
    assert snapshot(fresh, fresh.dwell(x[L:])) == second and second != want
    # two dwells enqueued back to back are never held back for one another: the fetch gives the second block's
    acq.dwell_enqueue(d_x.data_ptr(), st.cuda_stream)
    acq.dwell_enqueue(d_x.data_ptr() + 8 * L, st.cuda_stream)
    assert snapshot(acq, acq.fetch_results(st.cuda_stream)) == second
    # a ring, at a first index that is neither 0 nor even (the block is not 16-byte aligned there)
    ring = gnsscorr.IqStream(gctx, capacity_samples=4 * L, max_window_samples=L)
    ring.push(x)
    first = 1237
    assert snapshot(acq, acq.dwell_stream(ring, first)) == snapshot(fresh, fresh.dwell(x[first:]))
    ring.close()
    # cshort samples equal the float dwell of the converted samples
    q = np.clip(np.round(x[:L].view(np.float32) * 200.0), -32768, 32767).astype(np.int16)
    xf = q.astype(np.float32).view(np.complex64)
    float_run = snapshot(fresh, fresh.dwell(xf))
    acq.set_input_format(gnsscorr.GC_IQ_I16)
    d_q = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    assert snapshot(acq, acq.dwell_dev(d_q.data_ptr())) == float_run
    ring16 = gnsscorr.IqStream(gctx, capacity_samples=2 * L, max_window_samples=L, iq_format=gnsscorr.GC_IQ_I16)
    ring16.push(q.reshape(-1, 2))
    assert snapshot(acq, acq.dwell_stream(ring16, 0)) == float_run
    ring16.close()
    # cbyte
    q8 = np.clip(np.round(x[:L].view(np.float32) * 20.0), -128, 127).astype(np.int8)
    float_run8 = snapshot(fresh, fresh.dwell(q8.astype(np.float32).view(np.complex64)))
    acq.set_input_format(gnsscorr.GC_IQ_I8)
    d_q8 = torch.from_numpy(q8).cuda()
    torch.cuda.synchronize()
    assert snapshot(acq, acq.dwell_dev(d_q8.data_ptr())) == float_run8
    # reset: the grid reads as zeros until the next dwell
    acq.reset()
    assert not np.any(acq.grid(0))
    acq.close()
    fresh.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_usable(gctx, oracle):
    import gnsscorr
    N, f = 4000, 2
    lib = gnsscorr.load_library()
    x, _, code, ref = reference(oracle, N, f)
    c = _qs_conf(N, f)

    def refused(**kw):
        args = dict(c)
        ff = kw.pop("folding_factor", f)
        args.update(kw)
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=ff, **args)
        assert ei.value.status == gnsscorr.GC_ERR_INVALID, kw

    refused(folding_factor=0)
    refused(folding_factor=101)
    refused(folding_factor=60, samples_per_code=50.0)  # M = 50 // 60 < 1
    refused(sampled_ms=1)  # a block of 4000 samples is shorter than L = 8000
    refused(make_2_steps=True)
    with pytest.raises(ValueError):
        gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=f, combine="max", **c)
    # a raw handle comes back NULL
    conf = gnsscorr.AcqConf(N * 1000, 1, 1, float(N), float(N), 4, DMAX, DSTEP, 1, 0, 1, 0, 0, 4, 125.0)
    h = C.c_void_p()
    assert lib.gc_acq_create_quicksync(gctx._h, C.byref(conf), 1, 2, C.byref(h)) == gnsscorr.GC_ERR_INVALID and not h.value
    assert lib.gc_acq_create_quicksync(gctx._h, C.byref(conf), 0, 1, C.byref(h)) == gnsscorr.GC_ERR_INVALID and not h.value

    acq = gnsscorr.PcpsAcquisition(gctx, 1, folding_factor=f, **c)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        acq.dwell(x)  # no code yet
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    acq.set_local_code(0, code)
    for call in (lambda: acq.set_step_two(True, 0.0), lambda: acq.set_step_two(False), lambda: acq.set_frequency_offset(1000),
            lambda: acq.set_local_code_pair(0, np.tile(code, f), np.tile(code, f)), lambda: acq.set_local_code(1, code), lambda: acq.candidates(1),
            lambda: acq.peek(acq.PEEK_WIPEOFF, 5)):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            call()
        assert ei.value.status == gnsscorr.GC_ERR_INVALID
    # the candidates of a plain engine do not exist
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **_qs_conf(N, 1))
    delay, val = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    assert lib.gc_acq_quicksync_candidates(plain._h, 0, delay.ctypes.data_as(C.POINTER(C.c_uint32)), val.ctypes.data_as(C.POINTER(C.c_float))) == gnsscorr.GC_ERR_INVALID
    plain.close()
    # the engine works afterwards
    r = acq.dwell(x)[0]
    assert (r.indext, r.doppler_hz, r.acq_delay_samples) == (ref.indext, ref.doppler_hz, float(ref.acq_delay_samples))
    acq.close()
