"""GPU parity of the PCPS acquisition engine over the whole kernel matrix the planner can select (tests/acq_plan_ref.py; the CPU guard
tests/test_acq_plan.py keeps the matrix complete): every instantiated column size N1 with both store mappings of the forward
epilogues, every row kernel, the accumulate / two-dwell epilogues at every N1, and the first-vs-second-peak statistic with the
peak on every edge its kernel treats specially.  Same bars as tests/test_acquisition_gpu.py, whose helpers this file uses."""
import numpy as np
import pytest

from acq_plan_ref import DWELL_SIZES, LONG_ROW_SIZES, MATRIX_SIZES, plan
from test_acquisition_gpu import TOL, _check, _engine_against_oracle_everywhere

pytestmark = pytest.mark.gpu


def _size_conf(n, **kw):
    """One code period of GPS L1 C/A in n samples (fs = 1000 n), 4 Doppler bins."""
    fs = n * 1000
    return dict(fs_in=fs, sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=float(n),
        samples_per_chip=int(np.ceil(np.float32(9.7752e-07) * np.float32(fs))), doppler_max=1000, doppler_step=500, **kw)


def _every_stage_at_size(gctx, oracle, n):
    import gnsscorr
    from helpers import synth_stream
    fs = n * 1000
    chips = oracle.gps_l1_ca_code(9).astype(np.float32)
    x, truth = synth_stream([chips], fs, n, seed=n, cn0_db_hz=(50.0, 50.0), doppler_max=900.0)
    c = _size_conf(n)
    code = oracle.gps_l1_ca_code_sampled(9, fs)
    assert code.size == n
    acq = gnsscorr.PcpsAcquisition(gctx, 1, **c)
    assert (acq.fft_size, acq.num_doppler_bins) == (n, 4)
    acq.set_local_code(0, code)
    p = oracle.pcps(**c)
    p.set_local_code(code)
    r = _engine_against_oracle_everywhere(acq, p, x, (0, 3))
    expect = (-truth[0]["tau0"] * fs / 1.023e6) % n
    assert min(abs(r.indext - expect), n - abs(r.indext - expect)) <= n / 1023.0 + 1
    acq.close()


@pytest.mark.parametrize("n", MATRIX_SIZES, ids=["%d-n1_%d-%s" % (n, plan(n)[0], "perm" if plan(n)[3] else "plain") for n in MATRIX_SIZES])
def test_size_matrix_every_stage_against_oracle(gctx, oracle, n):
    """acq_cols_kernel<N1, INV, EPI> for all 17 N1, the forward epilogues with the plain and with the permuted lane-to-column
    mapping: wipe-off rows, spectra, code spectrum, whole grid, row maxima and result against the oracle."""
    _every_stage_at_size(gctx, oracle, n)


@pytest.mark.parametrize("n", LONG_ROW_SIZES)
def test_long_row_kernels_every_stage_against_oracle(gctx, oracle, n):
    """The stage lists of the packed row kernel for rows of 1600 to 4096 points (N1 = 32 / 50), which no size of the matrix reaches."""
    _every_stage_at_size(gctx, oracle, n)


@pytest.mark.parametrize("n", DWELL_SIZES, ids=["%d-n1_%d" % (n, plan(n)[0]) for n in DWELL_SIZES])
def test_dwell_epilogues_at_every_column_size(gctx, oracle, n):
    """Five non-coherent dwells, two satellites (one absent), first-vs-second-peak statistic.  (a) dwell() per block: MAG, then
    MAG_ACC four times; every dwell's result and the final grid against the oracle.  (b) after reset() the same blocks enqueued back
    to back: MAG2, MAG2_ACC and a trailing MAG_ACC.  A pair adds (grid + first) + second in the order two single passes add, so (b)
    equals (a) bit for bit."""
    import gnsscorr
    import torch
    from helpers import synth_stream
    fs, n_dwells = n * 1000, 5
    prns = (9, 21)
    x, _ = synth_stream([oracle.gps_l1_ca_code(prns[0]).astype(np.float32)], fs, n_dwells * n, seed=7000 + n, cn0_db_hz=(47.0, 47.0), doppler_max=900.0)
    c = _size_conf(n, max_dwells=n_dwells)
    acq = gnsscorr.PcpsAcquisition(gctx, len(prns), **c)
    assert (acq.fft_size, acq.num_doppler_bins) == (n, 4)
    orcs = []
    for s, prn in enumerate(prns):
        code = oracle.gps_l1_ca_code_sampled(prn, fs)
        acq.set_local_code(s, code)
        p = oracle.pcps(**c)
        p.set_local_code(code)
        orcs.append(p)
    for d in range(n_dwells):
        res_a = acq.dwell(x[d * n:])
        for s in range(len(prns)):
            q = orcs[s].core(x[d * n:])
            _check(res_a[s], q, cfar=False)
            assert res_a[s].second_peak == pytest.approx(q.second_peak, rel=TOL)
    grids_a = [acq.grid(s) for s in range(len(prns))]
    for s in range(len(prns)):
        ref = orcs[s].grid()
        assert np.max(np.abs(grids_a[s] - ref)) <= TOL * ref.max()
    assert res_a[0].test_statistics > 2.0 * res_a[1].test_statistics
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    acq.reset()
    for d in range(n_dwells):
        acq.dwell_enqueue(d_x.data_ptr() + 8 * n * d, st.cuda_stream)
    res_b = acq.fetch_results(st.cuda_stream)
    for s in range(len(prns)):
        g = acq.grid(s)
        assert np.array_equal(g, grids_a[s]), (s, np.max(np.abs(g - grids_a[s])))
        a_, b_ = res_a[s], res_b[s]
        assert (a_.indext, a_.doppler_index, a_.doppler_hz, a_.mag, a_.test_statistics, a_.second_peak, a_.second_peak_full_row) == \
            (b_.indext, b_.doppler_index, b_.doppler_hz, b_.mag, b_.test_statistics, b_.second_peak, b_.second_peak_full_row)
    acq.close()


def peak_targets(n, spc):
    """Code-phase indices at which acq_final_kernel does something else than in the middle of a row: the exclusion window wrapping
    below 0 or past N (with the reference's `else if`), the N / 4 floats its N-byte copy refreshes, the row pieces of ceil(N / 8)."""
    piece = -(-n // 8)
    t = [0, 1, spc - 1, spc, spc + 1, n // 4 - 1, n // 4, piece - 1, piece, 2 * piece, n - spc - 1, n - spc, n - spc + 1, n - 2, n - 1]
    return [v for i, v in enumerate(t) if 0 <= v < n and v not in t[:i]]  # spc = 1: N - spc + 1 is no index


PEAK_DOPPLER_BIN = 1  # -500 Hz of the (-1000, -500, 0, 500) grid


def peak_signal(code, n, t, seed):
    """The code delayed by t samples on the Doppler bin's own frequency, amplitude 1, plus complex noise 30 dB below the correlation
    peak: (a N)^2 against N sigma^2 after correlation, so sigma^2 = N / 1000."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i = np.arange(n)
    x = np.roll(code, t).astype(np.complex128) * np.exp(2j * np.pi * -500.0 * i / (n * 1000.0))
    sigma = np.sqrt(n / 1000.0)
    x += (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * sigma * np.sqrt(0.5)
    return x.astype(np.complex64)


@pytest.mark.parametrize("n,spc", [(4000, 4), (10000, 10), (1023, 1)])
def test_statistic_kernel_with_the_peak_on_every_edge(gctx, oracle, n, spc):
    """One engine and one oracle block search signals whose peak sits on each index of peak_targets() in turn, then the same in
    reverse order, with reset() between searches as a receiver does: the scratch row a search leaves behind is the next one's
    (d_tmp_buffer).  Index, Doppler and delay exact; magnitudes, both second peaks and the statistic to TOL / 2 TOL."""
    import gnsscorr
    fs = n * 1000
    c = _size_conf(n, use_cfar=False, max_dwells=1)
    c["samples_per_chip"] = spc
    code = oracle.gps_l1_ca_code_sampled(5, fs)
    acq = gnsscorr.PcpsAcquisition(gctx, 1, **c)
    acq.set_local_code(0, code)
    p = oracle.pcps(**c)
    p.set_local_code(code)
    targets = peak_targets(n, spc)
    for k, t in enumerate(targets + targets[::-1]):
        x = peak_signal(code, n, t, seed=100 * n + k)
        r, q = acq.dwell(x)[0], p.core(x)
        assert (q.indext, q.doppler_index) == (t, PEAK_DOPPLER_BIN), "the oracle's peak missed its target"
        assert r.indext == t, "search %d: peak at %d instead of %d" % (k, r.indext, t)
        _check(r, q, cfar=False)
        assert q.second_peak > 0.0 and q.second_peak_fixed > 0.0
        assert r.second_peak == pytest.approx(q.second_peak, rel=TOL), "search %d, peak at %d" % (k, t)
        assert r.second_peak_full_row == pytest.approx(q.second_peak_fixed, rel=TOL), "search %d, peak at %d" % (k, t)
        acq.reset()
        p.reset_grid()
    acq.close()
